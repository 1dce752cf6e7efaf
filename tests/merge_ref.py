"""The group merge of the reference restated twice: what pmmg_hip_merge_groups
is compared with (tests/test_gpu_merge.py), and what tests/test_merge_ref_host.py
holds against each other on the CPU.

  merge_seq()   PMMG_merge_grps steps 0-4 (reference src/mergemesh_pmmg.c:
                1004-1043: PMMG_mergeGrps_interfacePoints :433-469 with
                _addGrpJ :303-422, _internalPoints :480-571, _interfaceTetra
                :584-682, _internalTetra :695-751) transcribed loop by loop,
                with the fields the reference keeps its state in: point.tmp,
                tetra.flag / base, the two intvalues, the running np / ne of
                group 0
  merge_par()   the statement of include/parmmg_hip.h ("Group merge") in numpy
                array operations: first occurrences, stable order, prefix
                sums.  No loop over entities: the 1M-tetra case uses it.

Both take split_ref's output layout (a dict with count [ngrp, 4] = ne, np,
nface, nnode per group, tetv_out [sum ne, 4] with group-local ids, face_idx1/2,
node_idx1/2, groups concatenated; nnode_end / nface_end unless nnode / nface are
given) and return a dict of the C call's outputs: np, ne, new_pt [sum np],
new_tet [sum ne], src_pt [np], src_tet [ne], tetv_out [ne, 4], mark_out [ne]
(with color), node_val [nnode], face_val [nface].

Both assert the reference's two unchecked preconditions: within one group a
node position names one point, and a face position appears once.
"""
import numpy as np

KEYS = ("new_pt", "new_tet", "src_pt", "src_tet", "tetv_out", "node_val", "face_val")


def offsets(sp):
    """the four offset tables [ngrp + 1]: tetra, points, face entries, node entries"""
    c = np.asarray(sp["count"], np.int64).reshape(-1, 4)
    return np.concatenate([np.zeros((1, 4), np.int64), np.cumsum(c, axis=0)]).T


def _sizes(sp, nnode, nface):
    return (int(sp["nnode_end"] if nnode is None else nnode), int(sp["nface_end"] if nface is None else nface))


def merge_seq(sp, color=None, nnode=None, nface=None):
    te, pt, fa, no = (o.tolist() for o in offsets(sp))
    ngrp = len(te) - 1
    nnode, nface = _sizes(sp, nnode, nface)
    tetv = np.asarray(sp["tetv_out"]).reshape(-1, 4).tolist()
    n1, n2 = np.asarray(sp["node_idx1"]).tolist(), np.asarray(sp["node_idx2"]).tolist()
    f1, f2 = np.asarray(sp["face_idx1"]).tolist(), np.asarray(sp["face_idx2"]).tolist()
    for g in range(ngrp):  # the two preconditions
        seen = {}
        for k in range(no[g], no[g + 1]):
            assert seen.setdefault(n2[k], n1[k]) == n1[k], "a node position names two points of one group"
        pos = f2[fa[g]:fa[g + 1]]
        assert len(set(pos)) == len(pos), "a face position appears twice in one group"
    # group 0 is the merged mesh: its points and tetra keep their ids
    np_i, ne_i = pt[1], te[1]
    tet_i = [None] + [list(v) for v in tetv[:te[1]]]
    mark_i = [None] + [color[0] if color is not None else 0] * te[1]  # PMMG_set_color_tetra(parmesh, 0)
    src_pt, src_tet = list(range(1, np_i + 1)), list(range(1, ne_i + 1))
    node_int, face_int = [0] * nnode, [0] * nface  # the two intvalues (PMMG_CALLOC :994-999)
    tmp = [[0] * (pt[g + 1] - pt[g] + 1) for g in range(ngrp)]  # point.tmp of every group (:446-448)
    flag = [[0] * (te[g + 1] - te[g] + 1) for g in range(ngrp)]  # tetra.flag
    base = [[0] * (te[g + 1] - te[g] + 1) for g in range(ngrp)]  # tetra.base
    mesh_base = [0] * ngrp
    # step 0 :1006-1014
    for k in range(fa[0], fa[1]):
        face_int[f2[k]] = f1[k]
    # step 1: PMMG_mergeGrps_interfacePoints :452-466
    for k in range(no[0], no[1]):
        node_int[n2[k]] = n1[k]
    for g in range(1, ngrp):  # _addGrpJ :335-403
        for k in range(no[g], no[g + 1]):
            pos, ip = n2[k], n1[k]
            if tmp[g][ip]:
                continue
            if not node_int[pos]:
                np_i += 1  # MMG3D_newPt on a free list in order
                tmp[g][ip] = np_i
                node_int[pos] = np_i
                src_pt.append(pt[g] + ip)
            else:
                tmp[g][ip] = abs(node_int[pos])
                node_int[pos] *= -1
    for g in range(1, ngrp):
        # step 2: PMMG_mergeGrpJinI_internalPoints :505-552
        for k in range(1, pt[g + 1] - pt[g] + 1):
            if tmp[g][k]:
                continue
            np_i += 1
            tmp[g][k] = np_i
            src_pt.append(pt[g] + k)
        col = color[g] if color is not None else 0  # PMMG_set_color_tetra(parmesh, imsh): the group's marks

        def new_elt(iel):
            nonlocal ne_i
            ne_i += 1  # MMG3D_newElt on a free list in order
            tet_i.append([tmp[g][v] for v in tetv[te[g] + iel - 1]])
            mark_i.append(col)
            src_tet.append(te[g] + iel)
            return ne_i

        # step 3: PMMG_mergeGrpJinI_interfaceTetra :606-679
        mesh_base[g] += 1
        for k in range(fa[g], fa[g + 1]):
            pos = f2[k]
            iel, ifac, iploc = f1[k] // 12, (f1[k] % 12) // 3, (f1[k] % 12) % 3
            if base[g][iel] == mesh_base[g]:
                assert flag[g][iel]
                if not face_int[pos]:
                    face_int[pos] = 12 * flag[g][iel] + 3 * ifac + iploc
                else:
                    face_int[pos] *= -1
                continue
            base[g][iel] = mesh_base[g]
            ie = new_elt(iel)
            flag[g][iel] = ie
            if not face_int[pos]:
                face_int[pos] = 12 * ie + 3 * ifac + iploc
            else:
                face_int[pos] *= -1
        # step 4: PMMG_mergeGrpJinI_internalTetra :707-748
        for k in range(1, te[g + 1] - te[g] + 1):
            if base[g][k] == mesh_base[g]:
                continue
            base[g][k] = mesh_base[g]
            flag[g][k] = new_elt(k)  # (the reference leaves flag alone here; the call's new_tet names every tetra)
    new_pt = list(range(1, pt[1] + 1)) + [t for g in range(1, ngrp) for t in tmp[g][1:]]
    new_tet = list(range(1, te[1] + 1)) + [t for g in range(1, ngrp) for t in flag[g][1:]]
    i32 = lambda x: np.array(x, np.int32)
    out = dict(np=np_i, ne=ne_i, new_pt=i32(new_pt), new_tet=i32(new_tet), src_pt=i32(src_pt), src_tet=i32(src_tet),
               tetv_out=i32(tet_i[1:]).reshape(-1, 4), node_val=i32(node_int), face_val=i32(face_int))
    if color is not None:
        out["mark_out"] = i32(mark_i[1:])
    return out


def _first(keys):
    """(the distinct keys ascending, the index of the first occurrence of each)"""
    return np.unique(keys, return_index=True)


def merge_par(sp, color=None, nnode=None, nface=None):
    te, pt, fa, no = offsets(sp)
    ngrp = te.size - 1
    nnode, nface = _sizes(sp, nnode, nface)
    T, P, Ef, En = int(te[-1]), int(pt[-1]), int(fa[-1]), int(no[-1])
    tetv = np.asarray(sp["tetv_out"], np.int64).reshape(-1, 4)
    n1, n2 = np.asarray(sp["node_idx1"], np.int64), np.asarray(sp["node_idx2"], np.int64)
    f1, f2 = np.asarray(sp["face_idx1"], np.int64), np.asarray(sp["face_idx2"], np.int64)
    grp = lambda off: np.repeat(np.arange(ngrp), np.diff(off))
    gn, gf, gt, gp = grp(no), grp(fa), grp(te), grp(pt)
    for keys in (gn * (nnode + 1) + n2,):  # the two preconditions
        u, ui, inv = np.unique(keys, return_index=True, return_inverse=True)
        assert (n1[ui][inv.reshape(-1)] == n1).all(), "a node position names two points of one group"
    assert np.unique(gf * (nface + 1) + f2).size == Ef, "a face position appears twice in one group"
    np0, ne0 = int(pt[1]), int(te[1])
    # points: a point's entry is the first entry of its group's list that names it
    e = np.arange(En)
    pt_row = pt[gn] + n1 - 1  # the concatenated point an entry names
    ptfirst = np.full(P, -1, np.int64)
    later = e >= no[1]
    rows, idx = _first(pt_row[later])
    ptfirst[rows] = e[later][idx]
    holds = ~later | (ptfirst[pt_row] == e)  # every entry of group 0, the first entries of the others
    he = e[holds]
    posmin = np.full(nnode, -1, np.int64)
    ps, idx = _first(n2[he])
    posmin[ps] = he[idx]  # (he ascends)
    holders = np.bincount(n2[he[he >= no[1]]], minlength=nnode) + ((posmin >= 0) & (posmin < no[1]))
    creates = holds & later & (posmin[n2] == e)
    created_before = np.cumsum(creates) - creates
    ncre = int(creates.sum())
    pos_pt = np.zeros(nnode, np.int64)  # the merged point at every held position
    held = posmin >= 0
    e0 = posmin[held]
    pos_pt[held] = np.where(e0 < no[1], n1[e0], np0 + 1 + created_before[e0])
    unlisted = (np.arange(P) >= np0) & (ptfirst < 0)
    unl_before = np.cumsum(unlisted) - unlisted
    new_pt = np.where(np.arange(P) < np0, np.arange(P) + 1,
                      np.where(unlisted, np0 + ncre + 1 + unl_before, pos_pt[n2[np.maximum(ptfirst, 0)]] if En else 0))
    np_out = np0 + ncre + int(unlisted.sum())
    src_pt = np.zeros(np_out, np.int64)
    src_pt[:np0] = np.arange(1, np0 + 1)
    src_pt[np0 + created_before[creates]] = pt_row[creates] + 1
    src_pt[new_pt[unlisted] - 1] = np.nonzero(unlisted)[0] + 1
    node_val = np.where(held, pos_pt * np.where((holders - 1) % 2 == 1, -1, 1), 0)
    # tetra: the interface tetra of a group in order of their first entry, then the others in ascending id
    q = np.arange(Ef)
    laterf = q >= fa[1]
    tet_row = te[gf] + f1 // 12 - 1
    tetfirst = np.full(T, -1, np.int64)
    rows, idx = _first(tet_row[laterf])
    tetfirst[rows] = q[laterf][idx]
    firstf = laterf & (tetfirst[tet_row] == q)
    ft_before = np.concatenate([np.cumsum(firstf) - firstf, [int(firstf.sum())]])
    internal = (np.arange(T) >= ne0) & (tetfirst < 0)
    int_before = np.cumsum(internal) - internal
    n_ifc = ft_before[fa[gt + 1]] - ft_before[fa[gt]]  # the interface tetra of a tetra's group
    new_tet = np.where(np.arange(T) < ne0, np.arange(T) + 1,
                       np.where(internal, te[gt] + n_ifc + 1 + int_before - int_before[np.minimum(te[gt], T - 1)] if T else 0,
                                te[gt] + 1 + ft_before[np.maximum(tetfirst, 0)] - ft_before[fa[gt]]))
    src_tet = np.zeros(T, np.int64)
    src_tet[new_tet - 1] = np.arange(1, T + 1)
    tetv_out = np.zeros((T, 4), np.int64)
    tetv_out[new_tet - 1] = new_pt[(pt[gt][:, None] + tetv - 1)]
    # face values: the lowest entry's value, negated by every later entry of a group >= 1
    fmin = np.full(nface, -1, np.int64)
    ps, idx = _first(f2)
    fmin[ps] = idx
    named = fmin >= 0
    q0 = fmin[named]
    later_entries = np.bincount(f2[laterf], minlength=nface)[named] - (q0 >= fa[1])
    value = np.where(q0 < fa[1], f1[q0], 12 * new_tet[tet_row[q0]] + f1[q0] % 12 if T else 0)
    face_val = np.zeros(nface, np.int64)
    face_val[named] = value * np.where(later_entries % 2 == 1, -1, 1)
    i32 = lambda x: np.ascontiguousarray(x, np.int32)
    out = dict(np=np_out, ne=T, new_pt=i32(new_pt), new_tet=i32(new_tet), src_pt=i32(src_pt), src_tet=i32(src_tet),
               tetv_out=i32(tetv_out), node_val=i32(node_val), face_val=i32(face_val))
    if color is not None:
        mark = np.zeros(T, np.int64)
        mark[new_tet - 1] = np.asarray(color, np.int64)[gt]
        out["mark_out"] = i32(mark)
    return out


def assert_same(got, want, keys=KEYS):
    assert (got["np"], got["ne"]) == (want["np"], want["ne"])
    for k in keys + (("mark_out",) if "mark_out" in want else ()):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
