"""The contiguity code of the reference restated in numpy / Python: what the
device calls pmmg_hip_part_subgroups and pmmg_hip_fix_contiguity are compared
with (tests/test_gpu_contig.py), and the fixtures both test files share.

  subgroups()      connected components of the adjacency restricted to one
                   colour, by BFS; the table {color, head, size, exit}
  sweep_flags()    the `flag` PMMG_check_part_contiguity leaves
                   (src/metis_pmmg.c:321-387): colours in ascending order, a new
                   number at the first unseen node, ascending sweeps repeated
                   until nothing changes
  fix_flagged()    PMMG_fix_contiguity with its flag bookkeeping
                   (src/moveinterfaces_pmmg.c:228-299, :377-523), the choice of
                   the foreign neighbour pluggable: "bfs" is the reference's
                   (first in BFS order from the head), "lowest" the module's
                   (lowest (tetra, face))
  fix_free()       the statement of include/parmmg_hip.h without flags
  fix_oneshot()    every colour decided from the initial labelling (wrong: the
                   sequential dependency is real)

Arrays are 0-based rows of 1-based entities as everywhere in the tests: adja
[ne, 4] holds 4 k' + f' (k' 1-based) or 0; part [ne]; used [ne] bool or None.
"""
import functools
import heapq
from collections import deque

import numpy as np

from test_metis_graph import fixture


def nbrs(adja):
    """[ne, 4] neighbour rows (0-based), -1 where there is none"""
    a = np.asarray(adja)
    return np.where(a != 0, a // 4 - 1, -1).astype(np.int64)


def subgroups(adja, part, ncolor, used=None):
    """(head [ne] 1-based / 0 unused, flag [ne], ncomp [ncolor], table [nsub, 4] = color, head, size, exit in
    ascending head)"""
    nb = nbrs(adja)
    ne = nb.shape[0]
    part = np.zeros(ne, np.int32) if part is None else np.asarray(part)
    used = np.ones(ne, bool) if used is None else np.asarray(used)
    head = np.zeros(ne, np.int32)
    nbl = nb.tolist()
    pl = part.tolist()
    table = []
    for s in range(ne):
        if not used[s] or head[s]:
            continue
        c = pl[s]
        head[s] = s + 1
        q = deque([s])
        size = 0
        while q:
            k = q.popleft()
            size += 1
            for j in nbl[k]:
                if j >= 0 and not head[j] and pl[j] == c:
                    head[j] = s + 1
                    q.append(j)
        table.append([c, s + 1, size, 0])
    # exit: the lowest (tetra, face) whose neighbour has another colour
    foreign = (nb >= 0) & (part[np.where(nb >= 0, nb, 0)] != part[:, None]) & used[:, None]
    has = foreign.any(axis=1)
    cand = 4 * (np.arange(ne) + 1) + foreign.argmax(axis=1)
    best = np.full(ne + 1, np.iinfo(np.int64).max)
    np.minimum.at(best, head[has], cand[has])
    row = {}
    seen = [0] * ncolor
    flag = np.zeros(ne, np.int32)
    rank = np.zeros(ne + 1, np.int32)
    for i, r in enumerate(table):
        e = best[r[1]]
        r[3] = 0 if e == np.iinfo(np.int64).max else int(e)
        seen[r[0]] += 1
        rank[r[1]] = seen[r[0]]
        row[r[1]] = i
    flag[used] = rank[head[used]]
    return head, flag, np.array(seen, np.int32), np.array(table, np.int32).reshape(-1, 4)


def sweep_flags(adja, part, ncolor):
    """flag [ne] and the sweep count, by the loops of src/metis_pmmg.c:321-387 on the graph of adja.  One
    ascending sweep marks the unseen same-part neighbours of every node that carries the current number when the
    sweep reaches it: a node marked ahead of the sweep is reached in the same sweep, one marked behind it in the
    next.  The heap visits exactly those nodes in that order."""
    nb = nbrs(adja).tolist()
    ne = len(nb)
    part = np.zeros(ne, np.int32) if part is None else np.asarray(part)
    pl = part.tolist()
    flag = np.zeros(ne, np.int64)
    sweeps = 0
    for ipart in range(ncolor):
        mine = part == ipart
        ncolors = 0
        while True:
            unseen = mine & (flag == 0)
            if not unseen.any():
                break
            istart = int(unseen.argmax())  # the first node not seen
            ncolors += 1
            flag[istart] = ncolors
            now = [istart]
            while now:  # one sweep per turn, until a sweep marks nothing
                sweeps += 1
                heapq.heapify(now)
                later = []
                while now:
                    k = heapq.heappop(now)
                    for j in nb[k]:
                        if j >= 0 and pl[j] == ipart and flag[j] == 0:
                            flag[j] = ncolors
                            (heapq.heappush(now, j) if j > k else later.append(j))
                now = later
    return flag.astype(np.int32), sweeps


def _list_color(nbl, mark, flag, start, base, rule):
    """PMMG_list_contiguousColor: the BFS list from start over unflagged tetra of its colour, flagged base;
    the foreign neighbour by `rule`, or -1"""
    color = mark[start]
    lst = [start]
    flag[start] = base
    cur = 0
    while cur < len(lst):
        for j in nbl[lst[cur]]:
            if j >= 0 and not flag[j] and mark[j] == color:
                flag[j] = base
                lst.append(j)
        cur += 1
    for k in (lst if rule == "bfs" else sorted(lst)):
        for j in nbl[k]:
            if j >= 0 and flag[j] != base:
                return lst, j
    return lst, -1


def fix_flagged(adja, part, ncolor, rule, used=None):
    """PMMG_fix_contiguity for colours 0 .. ncolor-1: dict(part, nmoved, nmerged, nstuck)"""
    nbl = nbrs(adja).tolist()
    ne = len(nbl)
    used = np.ones(ne, bool) if used is None else np.asarray(used)
    mark = np.asarray(part).tolist()
    flag = [0 if u else -1 for u in used]  # (an unused tetra is never a start and never a neighbour)
    base = 0
    out = dict(nmoved=0, nmerged=0, nstuck=0)

    def merge(lst, o):
        for k in lst:
            mark[k] = mark[o]
            flag[k] = flag[o]
        out["nmoved"] += len(lst)
        out["nmerged"] += 1

    for color in range(ncolor):
        start = 0
        while start < ne and not (used[start] and mark[start] == color):
            start += 1
        if start >= ne:
            continue
        base += 1
        main, main_o = _list_color(nbl, mark, flag, start, base, rule)
        while True:
            start += 1
            while start < ne and not (flag[start] == 0 and mark[start] == color):
                start += 1
            if start >= ne:
                break
            base += 1
            nxt, nxt_o = _list_color(nbl, mark, flag, start, base, rule)
            if len(nxt) > len(main):
                if main_o < 0:
                    out["nstuck"] += 1
                else:
                    merge(main, main_o)
                    main, main_o = nxt, nxt_o
            elif nxt_o < 0:
                out["nstuck"] += 1
            else:
                merge(nxt, nxt_o)
    p = np.array(part, np.int32)
    p[used] = np.array(mark, np.int32)[used]
    out["part"] = p
    return out


def _decide(rows, part, adja):
    """the statement of include/parmmg_hip.h on one colour's rows (color, head, size, exit) in ascending head:
    (list of (row, colour it takes, replaced_main), nstuck)"""
    flat = np.asarray(adja).reshape(-1)
    across = lambda e: int(part[flat[e - 4] // 4 - 1])
    moves, nstuck = [], 0
    main = rows[0]
    for nxt in rows[1:]:
        if nxt[2] > main[2]:
            if main[3] == 0:
                nstuck += 1
            else:
                moves.append((main, across(main[3]), True))
                main = nxt
        elif nxt[3] == 0:
            nstuck += 1
        else:
            moves.append((nxt, across(nxt[3]), False))
    return moves, nstuck


def _fix_free(adja, part, ncolor, used, relabel):
    part = np.array(part, np.int32)
    initial = part.copy()
    out = dict(nmoved=0, nmerged=0, nstuck=0, moves=[])  # moves: (from colour, to colour, replaced_main)
    head, _, _, table = subgroups(adja, part, ncolor, used)
    for c in range(ncolor):
        if relabel and c:
            head, _, _, table = subgroups(adja, part, ncolor, used)
        rows = [r for r in table.tolist() if r[0] == c]
        if len(rows) < 2:
            continue
        moves, nstuck = _decide(rows, part if relabel else initial, adja)
        out["nstuck"] += nstuck
        for r, to, replaced in moves:
            part[head == r[1]] = to
            out["nmoved"] += r[2]
            out["nmerged"] += 1
            out["moves"].append((c, to, replaced))
    out["part"] = part
    return out


def fix_free(adja, part, ncolor, used=None):
    """for c ascending: the subgroups of colour c in the current part, decided, applied"""
    return _fix_free(adja, part, ncolor, used, True)


def fix_oneshot(adja, part, ncolor, used=None):
    """every colour decided from the initial labelling and the initial colours"""
    return _fix_free(adja, part, ncolor, used, False)


# ---------------------------------------------------------------- fixtures

def permuted(tetv, adja, perm):
    """the mesh with new tetra i = old tetra perm[i]"""
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.size)
    a = np.asarray(adja)[perm]
    out = np.where(a != 0, 4 * (inv[np.where(a != 0, a // 4 - 1, 0)] + 1) + a % 4, 0).astype(np.int32)
    return np.ascontiguousarray(np.asarray(tetv)[perm]), np.ascontiguousarray(out)


def _centroids(bg):
    c = bg.xyz[bg.tetv - 1].mean(axis=1)
    lo, hi = bg.xyz.min(axis=0), bg.xyz.max(axis=0)
    return (c - lo) / (hi - lo)


def _islands(u, part, ncolor, n, rng):
    for _ in range(n):
        c = rng.random(3)
        r = rng.uniform(0.05, 0.18)
        col = rng.integers(0, ncolor)
        part[np.linalg.norm(u - c, axis=1) < r] = col
    return part


def colours(case):
    """(part [6000] of the lattice fixture in its own numbering, ncolor)"""
    bg, _ = fixture()
    u = _centroids(bg)
    if case == "a":  # 4 slabs along x plus 12 spherical islands
        part = np.minimum((u[:, 0] * 4).astype(np.int32), 3)
        return _islands(u, part, 4, 12, np.random.default_rng(1)).astype(np.int32), 4
    if case == "b":  # 8 octants plus 40 islands
        o = (u >= 0.5).astype(np.int32)
        part = o[:, 0] + 2 * o[:, 1] + 4 * o[:, 2]
        return _islands(u, part, 8, 40, np.random.default_rng(2)).astype(np.int32), 8
    if case == "c":  # 3 colours drawn per tetra
        return np.random.default_rng(3).integers(0, 3, bg.ne).astype(np.int32), 3
    raise ValueError(case)


@functools.lru_cache(maxsize=None)
def mesh_case(case, scrambled):
    """dict(tetv, adja, part, ncolor, np) of the 6000-tetra lattice, lattice-numbered or with the tetra order
    permuted; read-only"""
    bg, _ = fixture()
    part, ncolor = colours(case)
    tetv, adja = np.array(bg.tetv), np.array(bg.adja)
    if scrambled:
        perm = np.random.default_rng(11).permutation(bg.ne)
        tetv, adja = permuted(tetv, adja, perm)
        part = np.ascontiguousarray(part[perm])
    for a in (tetv, adja, part):
        a.setflags(write=False)
    return dict(tetv=tetv, adja=adja, part=part, ncolor=ncolor, np=bg.np, xyz=bg.xyz)


MESH_CASES = [(c, s) for c in "abc" for s in (False, True)]


def path(order):
    """adja of a path through the tetra order[0], order[1], ... (0-based): each row's links are (previous, next,
    0, 0), and a link names the face of the neighbour that points back"""
    order = np.asarray(order, np.int64)
    a = np.zeros((order.size, 4), np.int32)
    a[order[1:], 0] = 4 * (order[:-1] + 1) + 1
    a[order[:-1], 1] = 4 * (order[1:] + 1) + 0
    return a


def blocks(*paths):
    """adja of several paths with no link between them, numbered one after the other"""
    out, base = [], 0
    for n in paths:
        a = path(np.arange(n))
        out.append(np.where(a != 0, a + 4 * base, 0))
        base += n
    return np.ascontiguousarray(np.vstack(out).astype(np.int32))


def tree(n, edges):
    """adja of a graph of n tetra with the links `edges` (0-based pairs, at most 4 per tetra): a tetra's faces
    are taken in the order of the list, and a link names the face of the neighbour that points back"""
    a = np.zeros((n, 4), np.int32)
    used = [0] * n
    for x, y in edges:
        fx, fy = used[x], used[y]
        a[x, fx], a[y, fy] = 4 * (y + 1) + fy, 4 * (x + 1) + fx
        used[x], used[y] = fx + 1, fy + 1
    return a


# Trees on which hook-and-flatten needs more rounds than ceil(log2 n) + 1: a root that is a local minimum of the
# root graph survives a round, so one round does not halve the roots.  Built like Fibonacci words, G(w+1) = G(w)
# and G(w-1) with their numbers interleaved and one link between them; 8, 34 and 55 tetra take 5, 8 and 9 rounds
# (hook_rounds() below), and the 55's one tetra with five links split in two gives 56 tetra with at most four.
TREES = {
    "tree8": (8, [(0, 4), (4, 3), (3, 7), (7, 5), (5, 6), (6, 1), (2, 7)]),
    "tree8b": (8, [(0, 7), (7, 4), (2, 6), (4, 6), (1, 5), (5, 3), (6, 3)]),
    "tree34": (34, [(0, 33), (33, 29), (16, 32), (29, 32), (8, 31), (31, 24), (32, 24), (4, 30), (30, 20), (12, 27),
                    (20, 27), (24, 27), (2, 28), (28, 18), (10, 26), (18, 26), (6, 22), (22, 14), (26, 14), (27, 14),
                    (1, 25), (25, 17), (9, 23), (17, 23), (5, 21), (21, 13), (23, 13), (3, 19), (19, 11), (7, 15),
                    (11, 15), (13, 15), (14, 15)]),
    "tree56": (56, [(0, 55), (55, 51), (33, 54), (51, 54), (17, 53), (53, 46), (54, 46), (8, 52), (52, 41), (25, 49),
                    (41, 49), (46, 49), (4, 50), (50, 37), (21, 48), (37, 48), (12, 44), (44, 29), (48, 29), (49, 29),
                    (2, 47), (47, 35), (19, 45), (35, 45), (10, 43), (43, 27), (45, 27), (6, 39), (39, 23), (14, 16),
                    (23, 31), (27, 31), (29, 31), (1, 42), (42, 34), (18, 40), (34, 40), (9, 38), (38, 26), (40, 26),
                    (5, 36), (36, 22), (13, 30), (22, 30), (26, 30), (3, 32), (32, 20), (11, 28), (20, 28), (7, 24),
                    (24, 15), (28, 15), (30, 15), (15, 16), (31, 16)]),
}
TREE_ROUNDS = {"tree8": 5, "tree8b": 5, "tree34": 8, "tree56": 9}


def hook_rounds(adja, part=None):
    """Hooking rounds of the device's labelling scheme with round by round (a round on the device reads only the
    labels of its start, so this is the device's round count exactly): the first round leaves every tetra at its
    lowest same-colour neighbour below it; each later one flattens, then hooks the higher root of every
    same-colour link below the lower (the minimum wins); the round that hooks nothing is counted.  Returns
    (rounds, labels = the lowest tetra of each subgroup, 0-based)."""
    nb = nbrs(adja)
    ne = nb.shape[0]
    part = np.zeros(ne, np.int32) if part is None else np.asarray(part)
    k, f = np.nonzero(nb >= 0)
    j = nb[k, f]
    same = part[k] == part[j]
    k, j = k[same], j[same]
    L = np.arange(ne)
    np.minimum.at(L, k, j)
    rounds = 1
    while True:
        while True:  # flatten
            g = L[L]
            if (g == L).all():
                break
            L = g
        lk, lj = L[k], L[j]
        d = lk != lj
        rounds += 1
        if not d.any():
            return rounds, L
        L = L.copy()
        np.minimum.at(L, np.maximum(lk, lj)[d], np.minimum(lk, lj)[d])


def round_bound(ne):
    """what the scheme is proven to stay within: a root that survives two consecutive rounds absorbed a root of
    its own in the first, so the roots halve every two rounds; with the idle last round 2 ceil(log2 ne) + 1"""
    return 2 * int(np.ceil(np.log2(max(ne, 2)))) + 1


@functools.lru_cache(maxsize=None)
def graph_case(name):
    """dict(adja, part | None, ncolor) of a pure-adjacency graph (no vertices); read-only"""
    P = lambda *c: np.array(c, np.int32)
    if name == "path7":  # the sequential dependency: 5 moves to colour 1 and bridges {4} and {6, 7}
        g = dict(adja=path(np.arange(7)), part=P(0, 0, 0, 1, 0, 1, 1), ncolor=2)
    elif name == "equal":  # two subgroups of one size: main stays the lower head
        g = dict(adja=path(np.arange(5)), part=P(0, 0, 1, 0, 0), ncolor=2)
    elif name == "stuck":  # main {1, 2} touches nothing; {3, 4, 5} is larger: nothing moves
        g = dict(adja=blocks(2, 4), part=P(0, 0, 0, 0, 0, 1), ncolor=2)
    elif name == "stuck_later":  # ... and {7, 8, 9} is compared with the old main's size: stuck too; {12} moves
        g = dict(adja=blocks(2, 10), part=P(0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 1), ncolor=2)
    elif name == "two_blocks":  # no link between the colours: exit 0, nothing to fix
        g = dict(adja=blocks(3, 4), part=P(0, 0, 0, 1, 1, 1, 1), ncolor=2)
    elif name == "empty_colour":  # colour 1 of 3 has no tetra
        g = dict(adja=path(np.arange(6)), part=P(0, 0, 2, 2, 0, 2), ncolor=3)
    elif name in TREES:
        g = dict(adja=tree(*TREES[name]), part=None, ncolor=1)
    elif name.startswith("scrambled"):  # scrambled<n>_one / scrambled<n>_bands
        n = int(name[len("scrambled"):name.index("_")])
        order = np.random.default_rng(n).permutation(n)
        part = None
        if name.endswith("_bands"):  # bands of 64 along the path, colours alternating
            part = np.empty(n, np.int32)
            part[order] = (np.arange(n) // 64) % 2
        g = dict(adja=path(order), part=part, ncolor=1 if part is None else 2)
    else:
        raise ValueError(name)
    for a in g.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return g


SMALL_GRAPHS = ["path7", "equal", "stuck", "stuck_later", "two_blocks", "empty_colour"]
TREE_GRAPHS = ["tree8", "tree8b", "tree34", "tree56"]
PATH_GRAPHS = ["scrambled4097_one", "scrambled4097_bands", "scrambled65537_one", "scrambled65537_bands"]
