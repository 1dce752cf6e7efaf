"""The group split of the reference restated twice: what pmmg_hip_split_groups
is compared with (tests/test_gpu_split.py), and what tests/test_split_ref_host.py
holds against each other on the CPU.

  split_seq()   PMMG_split_eachGrp and PMMG_splitGrps_fillGroup (reference
                src/grpsplit_pmmg.c:1267-1445, :819-1094) transcribed loop by
                loop, with the fields the reference keeps its state in:
                tetra.flag, point.s, point.flag, point.tmp,
                posInIntFaceComm / iplocFaceComm and the two nitem counters
  split_par()   the statement of include/parmmg_hip.h ("Group split") in numpy
                array operations: a stable sort by colour, first occurrences,
                prefix sums.  No loop over tetra: the 1M-tetra case uses it.

Both take rows of 1-based entities (tetv [ne, 4], adja [ne, 4] = 4 k' + f' or
0, part [ne]) and return a dict of the C call's outputs: count [ngrp, 4] = ne,
np, nface, nnode per group; old_tet, new_tet [ne]; tetv_out, adja_out [ne, 4];
old_pt; face_idx1/2; node_idx1/2; nnode_end, nface_end.
"""
import numpy as np

IDIR = np.array([[1, 2, 3], [0, 3, 2], [0, 1, 3], [0, 2, 1]])  # MMG5_idir
UNSET = -1

KEYS = ("count", "old_tet", "new_tet", "tetv_out", "adja_out", "old_pt", "face_idx1", "face_idx2", "node_idx1",
        "node_idx2")


def split_seq(tetv, adja, part, ngrp, npv, node_pos=None, face_old=None, nnode0=0, nface0=0):
    tetv, adja, part = np.asarray(tetv).tolist(), np.asarray(adja).tolist(), np.asarray(part).tolist()
    ne = len(tetv)
    idir = IDIR.tolist()
    # PMMG_splitGrps_countTetPerGrp :1114: countPerGrp, and tetra.flag = the id inside the group
    count_per_grp = [0] * ngrp
    flag = [0] * (ne + 1)
    for tet in range(1, ne + 1):
        count_per_grp[part[tet - 1]] += 1
        flag[tet] = count_per_grp[part[tet - 1]]
    # PMMG_split_eachGrp :1292-1325
    pos_in_comm = [UNSET] * (4 * ne + 1)
    iploc_comm = [UNSET] * (4 * ne + 1)
    if face_old is not None:
        fo = np.asarray(face_old).reshape(-1).tolist()
        for k in range(ne):
            for f in range(4):
                if fo[4 * k + f] >= 0:
                    pos_in_comm[4 * k + 1 + f] = fo[4 * k + f] // 3
                    iploc_comm[4 * k + 1 + f] = fo[4 * k + f] % 3
    p_tmp = [UNSET] * (npv + 1)
    p_s = [UNSET] * (npv + 1)
    p_flag = [0] * (npv + 1)
    if node_pos is not None:
        p_tmp[1:] = np.asarray(node_pos).tolist()
    node_nitem, face_nitem = nnode0, nface0
    # :1343-1348: the old id of every new tetra
    new_flag = [[0] * (count_per_grp[g] + 1) for g in range(ngrp)]
    for ie in range(1, ne + 1):
        new_flag[part[ie - 1]][flag[ie]] = ie
    out = dict(count=np.zeros((ngrp, 4), np.int32), old_tet=[], tetv_out=[], adja_out=[], old_pt=[], face_idx1=[],
               face_idx2=[], node_idx1=[], node_idx2=[])
    for grp in range(ngrp):
        n = count_per_grp[grp]
        np_new = 0
        g_v = [[0] * 4 for _ in range(n + 1)]
        g_adja = [[0] * 4 for _ in range(n + 1)]
        pt_tmp = [UNSET]  # the new points' tmp (a copy of the old point's at the time it was added)
        old_pt, f1, f2, n1, n2 = [], [], [], [], []
        for t in range(1, n + 1):  # PMMG_splitGrps_fillGroup :849
            tet = new_flag[grp][t]
            v = tetv[tet - 1]
            for poi in range(4):  # :879
                if p_s[v[poi]] != grp:
                    np_new += 1
                    pt_tmp.append(p_tmp[v[poi]])
                    old_pt.append(v[poi])
                    g_v[t][poi] = np_new
                    p_s[v[poi]] = grp
                    p_flag[v[poi]] = np_new
                    if pt_tmp[np_new] != UNSET:  # PMMG_splitGrps_updateNodeCommOld :659
                        n1.append(np_new)
                        n2.append(pt_tmp[np_new])
                        node_nitem += 1
                else:
                    g_v[t][poi] = p_flag[v[poi]]
            g_adja[t] = list(adja[tet - 1])  # :1009
            for fac in range(4):  # :1012
                pos = 4 * (tet - 1) + 1 + fac
                if g_adja[t][fac] == 0:  # PMMG_splitGrps_updateFaceCommOld :774
                    if pos_in_comm[pos] >= 0:
                        f1.append(12 * t + 3 * fac + iploc_comm[pos])
                        f2.append(pos_in_comm[pos])
                    continue
                adjidx, vidx = g_adja[t][fac] // 4, g_adja[t][fac] % 4
                if part[adjidx - 1] != grp:  # :1023
                    g_adja[t][fac] = 0
                    other = 4 * (adjidx - 1) + 1 + vidx
                    if pos_in_comm[other] < 0:  # PMMG_splitGrps_updateFaceCommNew :704
                        pos_in_comm[pos] = pos_in_comm[other] = face_nitem
                        ip = v[idir[fac][0]]
                        iplocadj = [tetv[adjidx - 1][idir[vidx][j]] for j in range(3)].index(ip)
                        iploc_comm[pos], iploc_comm[other] = 0, iplocadj
                        f1.append(12 * t + 3 * fac + 0)
                        f2.append(pos_in_comm[pos])
                        face_nitem += 1
                    else:
                        f1.append(12 * t + 3 * fac + iploc_comm[pos])
                        f2.append(pos_in_comm[pos])
                elif adjidx < tet:  # :1066
                    g_adja[t][fac] = 4 * flag[adjidx] + vidx
                    g_adja[flag[adjidx]][vidx] = 4 * t + fac
        for t in range(1, n + 1):  # :1081, PMMG_splitGrps_updateNodeCommNew :606
            tet = new_flag[grp][t]
            for fac in range(4):
                adjidx = adja[tet - 1][fac] // 4
                if adjidx and grp != part[adjidx - 1]:
                    for poi in range(3):
                        ip = g_v[t][idir[fac][poi]]
                        if pt_tmp[ip] == UNSET:
                            n1.append(ip)
                            n2.append(node_nitem + 1)
                            p_tmp[tetv[tet - 1][idir[fac][poi]]] = node_nitem + 1
                            pt_tmp[ip] = node_nitem + 1
                            node_nitem += 1
        out["count"][grp] = (n, np_new, len(f1), len(n1))
        out["old_tet"] += new_flag[grp][1:]
        out["tetv_out"] += g_v[1:]
        out["adja_out"] += g_adja[1:]
        for k, lst in (("old_pt", old_pt), ("face_idx1", f1), ("face_idx2", f2), ("node_idx1", n1), ("node_idx2", n2)):
            out[k] += lst
    for k in ("old_tet", "old_pt", "face_idx1", "face_idx2", "node_idx1", "node_idx2"):
        out[k] = np.array(out[k], np.int32).reshape(-1)
    for k in ("tetv_out", "adja_out"):
        out[k] = np.array(out[k], np.int32).reshape(-1, 4)
    out["new_tet"] = np.array(flag[1:], np.int32)
    out["nnode_end"], out["nface_end"] = node_nitem, face_nitem
    return out


def split_par(tetv, adja, part, ngrp, npv, node_pos=None, face_old=None, nnode0=0, nface0=0):
    tetv, adja, part = np.asarray(tetv, np.int64), np.asarray(adja, np.int64), np.asarray(part, np.int64)
    ne = tetv.shape[0]
    node_pos = np.full(npv, -1, np.int64) if node_pos is None else np.asarray(node_pos, np.int64)
    face_old = np.full((ne, 4), -1, np.int64) if face_old is None else np.asarray(face_old, np.int64).reshape(ne, 4)
    # tetra: a stable sort by colour; n = a tetra's place over all groups
    order = np.argsort(part, kind="stable")
    place = np.empty(ne, np.int64)
    place[order] = np.arange(ne)
    teoff = np.searchsorted(part[order], np.arange(ngrp + 1))
    g = part[order]
    new_tet = place - teoff[part] + 1
    # points: the first corner, in place order, of every (colour, vertex)
    vq = tetv[order].reshape(-1)
    gq = np.repeat(g, 4)
    _, first_idx, inv = np.unique(gq * (npv + 1) + vq, return_index=True, return_inverse=True)
    first = first_idx[inv.reshape(-1)]
    is_first = first == np.arange(4 * ne)
    pt_before = np.cumsum(is_first) - is_first  # points before a corner, over all groups
    pt_total = int(is_first.sum())
    pt_off = np.concatenate([pt_before, [pt_total]])[4 * teoff]
    tetv_out = (pt_before[first] - pt_off[gq] + 1).reshape(ne, 4)
    old_pt = vq[is_first]
    # adjacency
    a = adja[order]
    has = a != 0
    j = np.where(has, a // 4 - 1, 0)
    gj = np.where(has, part[j], -1)
    inside = has & (gj == g[:, None])
    adja_out = np.where(inside, 4 * new_tet[j] + a % 4, 0)
    # faces, in (n, f) order
    outward = has & ~inside
    own = outward & (gj > g[:, None])
    old_face = ~has & (face_old[order] >= 0)
    ent = outward | old_face
    num = nface0 + (np.cumsum(own) - own.reshape(-1)).reshape(ne, 4)  # an owned face's number
    t_loc = (np.arange(ne) - teoff[g] + 1)[:, None]
    f_ix = np.arange(4)[None, :]
    nj = place[j]
    num_other = num[nj, a % 4]
    v_new = tetv[order]
    ip = tetv[j, IDIR[a % 4, 0]]  # the owner's v[MMG5_idir[i][0]]
    mine = v_new[:, IDIR]  # [ne, 4 faces, 3]
    iploc_other = (mine == ip[:, :, None]).argmax(axis=2)
    fo = face_old[order]
    iploc = np.where(old_face, fo % 3, np.where(own, 0, iploc_other))
    idx2 = np.where(old_face, fo // 3, np.where(own, num, num_other))
    idx1 = 12 * t_loc + 3 * f_ix + iploc
    face_idx1, face_idx2 = idx1[ent], idx2[ent]
    nface = np.concatenate([[0], np.cumsum(ent.sum(axis=1))])[teoff]
    # nodes: the owner of a vertex without a position is the lowest (n, f, p) over the outward faces
    n_ix, f_idx = np.nonzero(outward)
    key = (12 * n_ix[:, None] + 3 * f_idx[:, None] + np.arange(3)[None, :]).reshape(-1)
    vert = v_new[n_ix[:, None], IDIR[f_idx]].reshape(-1)
    keep = node_pos[vert - 1] < 0
    key, vert = key[keep], vert[keep]
    owner_key = np.full(npv + 1, -1, np.int64)
    uv, ui = np.unique(vert, return_index=True)  # (key ascends with the index)
    owner_key[uv] = key[ui]
    owner_col = np.where(owner_key >= 0, g[np.maximum(owner_key, 0) // 12] if ne else 0, ngrp)
    run2_key = np.sort(owner_key[uv])  # ascending (colour, n, f, p)
    run2_n = run2_key // 12
    run2_g = g[run2_n] if ne else run2_n
    run2_v = v_new.reshape(-1)[4 * run2_n + IDIR[(run2_key % 12) // 3, run2_key % 3]]
    c2 = np.bincount(run2_g, minlength=ngrp)[:ngrp]
    # run 1: the points of a group that came with a position or got one from a lower colour
    fq = np.nonzero(is_first)[0]
    run1 = (node_pos[vq[fq] - 1] >= 0) | (owner_col[vq[fq]] < gq[fq])
    r1_q = fq[run1]
    r1_g = gq[r1_q]
    c1 = np.bincount(r1_g, minlength=ngrp)[:ngrp]
    c1_off = np.concatenate([[0], np.cumsum(c1)])
    c2_off = np.concatenate([[0], np.cumsum(c2)])
    at1 = c2_off[r1_g] + np.arange(r1_q.size)  # place in the concatenated list
    at2 = c1_off[run2_g + 1] + np.arange(run2_key.size)
    total = int(c1.sum() + c2.sum())
    vpos = np.full(npv + 1, -1, np.int64)
    vpos[1:] = node_pos
    vpos[run2_v] = nnode0 + at2 + 1  # nitem + 1, nitem counting the entries appended so far
    node_idx1 = np.zeros(total, np.int64)
    node_idx2 = np.zeros(total, np.int64)
    node_idx1[at1] = pt_before[r1_q] - pt_off[r1_g] + 1
    node_idx2[at1] = vpos[vq[r1_q]]
    q2 = 4 * run2_n + IDIR[(run2_key % 12) // 3, run2_key % 3]
    node_idx1[at2] = tetv_out.reshape(-1)[q2]
    node_idx2[at2] = nnode0 + at2 + 1
    count = np.stack([np.diff(teoff), np.diff(pt_off), np.diff(nface), c1 + c2], axis=1)
    i32 = lambda x: np.ascontiguousarray(x, np.int32)
    return dict(count=i32(count), old_tet=i32(order + 1), new_tet=i32(new_tet), tetv_out=i32(tetv_out),
                adja_out=i32(adja_out), old_pt=i32(old_pt), face_idx1=i32(face_idx1), face_idx2=i32(face_idx2),
                node_idx1=i32(node_idx1), node_idx2=i32(node_idx2), nnode_end=nnode0 + total,
                nface_end=nface0 + int(own.sum()))


def old_positions(tetv, adja, seed):
    """(node_pos [np], face_old [ne, 4], nnode0, nface0): random old communicator positions on half the boundary
    faces and on their vertices, as a group that already had parallel faces would bring them"""
    tetv, adja = np.asarray(tetv), np.asarray(adja)
    rng = np.random.default_rng(seed)
    npv = int(tetv.max())
    k, f = np.nonzero(adja == 0)
    pick = rng.random(k.size) < 0.5
    k, f = k[pick], f[pick]
    face_old = np.full(adja.shape, -1, np.int32)
    face_old[k, f] = 3 * rng.permutation(k.size) + rng.integers(0, 3, k.size)
    verts = np.unique(tetv[k[:, None], IDIR[f]])
    node_pos = np.full(npv, -1, np.int32)
    node_pos[verts - 1] = rng.permutation(verts.size) + 1
    return node_pos, face_old, int(verts.size), int(k.size)


def segments(out):
    """the four offset tables [ngrp + 1] of an output: tetra, points, face entries, node entries"""
    z = np.zeros((1, 4), np.int64)
    return np.concatenate([z, np.cumsum(out["count"].astype(np.int64), axis=0)]).T


def assert_same(got, want, keys=KEYS):
    for k in keys:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert (got["nnode_end"], got["nface_end"]) == (want["nnode_end"], want["nface_end"])
