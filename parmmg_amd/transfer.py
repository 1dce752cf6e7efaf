"""Python front-end of the C-ABI (include/parmmg_hip.h) and of the C host
layer (csrc/pmmg_host.h).

``TransferContext`` wraps one ``pmmg_hip_ctx``.  Host-mode calls take numpy
arrays; device-mode calls take ``DeviceArray`` handles (raw HIP allocations
made through the module itself), which is what the benchmark uses to keep
every input resident in HBM.

``interp_metrics_and_fields`` mirrors the reference driver
``PMMG_interpMetricsAndFields(parmesh, permNodGlob)``
(src/interpmesh_pmmg.c:663-741) group by group, through the C host layer.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from ._native import HipGroup, HipLenHisto, HipQualHisto, HipSplitCount, HipStats, HipSubgroup, hip_lib, host_lib

HOST, DEVICE = 0, 1
PT_SKIP, PT_VOL, PT_BDY = 0, 1, 2

HIT_NAMES = {
    0: "none", 1: "vol_walk", 2: "vol_exhaust", 3: "vol_closest", 4: "bdy_face", 5: "bdy_edge", 6: "bdy_vertex",
    7: "bdy_wedge", 8: "bdy_cone", 9: "bdy_exhaust", 10: "bdy_stale", 11: "bdy_closest",
}


def _p(a):
    if a is None:
        return None
    if isinstance(a, DeviceArray):
        return ctypes.c_void_p(a.ptr)
    if getattr(a, "is_cuda", False):  # torch tensor in HBM (e.g. an all-gather buffer)
        if not a.is_contiguous():
            raise ValueError("device tensors passed to the C-ABI must be contiguous")
        return ctypes.c_void_p(a.data_ptr())
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError("arrays passed to the C-ABI must be C-contiguous")
    return a.ctypes.data_as(ctypes.c_void_p)


def _is_dev(a) -> bool:
    return isinstance(a, DeviceArray) or bool(getattr(a, "is_cuda", False))


def _free_all(arrays) -> None:
    """the outputs a failed call allocated (None: one that was not asked for)"""
    for a in arrays:
        if a is not None:
            a.free()


@dataclass
class DeviceArray:
    ptr: int
    nbytes: int
    shape: tuple
    dtype: np.dtype
    ctx: "TransferContext"

    def download(self) -> np.ndarray:
        out = np.empty(self.shape, self.dtype)
        if not self.ctx.lib.pmmg_hip_memcpy_d2h(self.ctx.h, _p(out), ctypes.c_void_p(self.ptr), self.nbytes):
            raise RuntimeError(self.ctx.error())
        return out

    def zero(self) -> None:
        z = np.zeros(self.nbytes, np.uint8)
        if not self.ctx.lib.pmmg_hip_memcpy_h2d(self.ctx.h, ctypes.c_void_p(self.ptr), _p(z), self.nbytes):
            raise RuntimeError(self.ctx.error())

    def free(self) -> None:
        if self.ptr:
            self.ctx.lib.pmmg_hip_free(self.ctx.h, ctypes.c_void_p(self.ptr))
            self.ptr = 0


def device_count() -> int:
    return int(hip_lib().pmmg_hip_device_count())


def pack_tet8(tetv: np.ndarray, adja: np.ndarray) -> np.ndarray:
    """Packed tetra records {v0..v3, adja0..adja3} (include/parmmg_hip.h,
    pmmg_hip_set_background_tet8): what a host shim builds while packing
    MMG5_Tetra.v."""
    return np.ascontiguousarray(np.hstack([np.asarray(tetv, np.int32), np.asarray(adja, np.int32)]))


def pack_solutions(met, fields) -> np.ndarray:
    """Packed per-vertex solution records [metric | field 0 | ...], stride
    rounded up to an even number of doubles (include/parmmg_hip.h,
    pmmg_hip_set_solutions_packed)."""
    cols = ([] if met is None else [np.asarray(met, np.float64)]) + [np.asarray(f, np.float64) for f in fields]
    k = sum(c.shape[1] for c in cols)
    rs = (k + 1) & ~1
    rec = np.zeros((cols[0].shape[0], rs), np.float64)
    o = 0
    for c in cols:
        rec[:, o:o + c.shape[1]] = c
        o += c.shape[1]
    return rec


class TransferContext:
    """One ``pmmg_hip_ctx`` on a HIP device."""

    def __init__(self, device: int = 0, sort: bool | None = None):
        """sort=None picks the query order on the device (Morton-bin unless
        the numbering is spatially coherent); True / False force binning /
        input order."""
        self.lib = hip_lib()
        opts = 0 if sort is None else (2 if sort else 1)
        self.h = self.lib.pmmg_hip_create(int(device), opts)
        if not self.h:
            raise RuntimeError(f"pmmg_hip_create({device}) failed: no usable HIP device (the transfer step has "
                               "no CPU fallback)")
        self._keep: list = []

    def close(self) -> None:
        if self.h:
            self.lib.pmmg_hip_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def error(self) -> str:
        e = self.lib.pmmg_hip_last_error(self.h)
        return e.decode() if e else ""

    def _ck(self, ok: int, what: str) -> None:
        if not ok:
            raise RuntimeError(f"{what} failed: {self.error()}")

    # ------------------------------------------------------------------ device memory
    def upload(self, a: np.ndarray) -> DeviceArray:
        a = np.ascontiguousarray(a)
        ptr = self.lib.pmmg_hip_malloc(self.h, a.nbytes)
        if not ptr:
            raise RuntimeError(self.error())
        self._ck(self.lib.pmmg_hip_memcpy_h2d(self.h, ctypes.c_void_p(ptr), _p(a), a.nbytes), "h2d")
        return DeviceArray(ptr, a.nbytes, a.shape, a.dtype, self)

    def empty(self, shape, dtype) -> DeviceArray:
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        ptr = self.lib.pmmg_hip_malloc(self.h, nbytes)
        if not ptr:
            raise RuntimeError(self.error())
        return DeviceArray(ptr, nbytes, tuple(shape), dtype, self)

    # ------------------------------------------------------------------ C-ABI
    def set_background(self, xyz, tetv, adja, triv, adjt, hausd: float) -> None:
        """adja None: adjacency built on the device; triv None: boundary trias
        and their adjacency built on the device; adjt None (triv given): tria
        adjacency built on the device."""
        where = DEVICE if _is_dev(xyz) else HOST
        npt, ne, nt = xyz.shape[0], tetv.shape[0], (-1 if triv is None else triv.shape[0])
        self._keep = [xyz, tetv, adja, triv, adjt]
        self._ck(self.lib.pmmg_hip_set_background(self.h, npt, _p(xyz), ne, _p(tetv), _p(adja), nt, _p(triv),
                                                  _p(adjt), float(hausd), where), "set_background")

    def set_background_tet8(self, xyz, tet8, triv, adjt, hausd: float) -> None:
        """Background with packed {v[4], adja[4]} tetra records (pack_tet8)."""
        where = DEVICE if _is_dev(xyz) else HOST
        npt, ne, nt = xyz.shape[0], tet8.shape[0], triv.shape[0]
        if tet8.shape[1] != 8:
            raise ValueError("tet8 must have 8 ints per tetra")
        self._keep = [xyz, tet8, triv, adjt]
        self._ck(self.lib.pmmg_hip_set_background_tet8(self.h, npt, _p(xyz), ne, _p(tet8), nt, _p(triv), _p(adjt),
                                                       float(hausd), where), "set_background_tet8")

    # ------------------------------------------------------------------ background snapshot
    def build_adjacency(self, npt: int, tetv: DeviceArray, adja: bool = True, tet8: bool = True, out=None):
        """Device-side MMG3D_hashTetra: (adja, tet8) DeviceArrays (None when
        not requested); out = (adja, tet8) arrays to fill instead of new ones."""
        ne = tetv.shape[0]
        a = (out[0] if out and out[0] is not None else self.empty((ne, 4), np.int32)) if adja else None
        t = (out[1] if out and out[1] is not None else self.empty((ne, 8), np.int32)) if tet8 else None
        self._ck(self.lib.pmmg_hip_build_adjacency(self.h, int(npt), ne, _p(tetv), _p(a), _p(t)), "build_adjacency")
        return a, t

    def build_boundary(self, npt: int, tet8: DeviceArray | None = None, tetv: DeviceArray | None = None,
                       adja: DeviceArray | None = None, adjt: bool = True, tref: DeviceArray | None = None):
        """Device-side MMG5_chkBdryTria + MMG3D_hashTria: (triv, adjt) DeviceArrays of nt rows
        (tref: tetra references, for interface faces of a multi-material mesh)."""
        ne = (tet8 if tet8 is not None else tetv).shape[0]
        nt = ctypes.c_int(0)
        # capacity 0: the call only counts (it fails when there are trias, with nt set)
        self.lib.pmmg_hip_build_boundary(self.h, int(npt), ne, _p(tet8), _p(tetv), _p(adja), _p(tref), 0,
                                         ctypes.byref(nt), None, None)
        n = nt.value
        triv = self.empty((n, 3), np.int32)
        at = self.empty((n, 3), np.int32) if adjt else None
        self._ck(self.lib.pmmg_hip_build_boundary(self.h, int(npt), ne, _p(tet8), _p(tetv), _p(adja), _p(tref), n,
                                                  ctypes.byref(nt), _p(triv), _p(at)), "build_boundary")
        return triv, at

    def set_solutions(self, met, fields) -> None:
        fields = list(fields)
        where = DEVICE if (_is_dev(met) or (fields and _is_dev(fields[0]))) else HOST
        msize = 0 if met is None else int(met.shape[1])
        sizes = (ctypes.c_int * max(1, len(fields)))(*[int(f.shape[1]) for f in fields])
        ptrs = (ctypes.c_void_p * max(1, len(fields)))(*[_p(f) for f in fields])
        self._sol_keep = [met, fields, sizes, ptrs]
        self._ck(self.lib.pmmg_hip_set_solutions(self.h, msize, _p(met), len(fields), sizes, ptrs, where),
                 "set_solutions")

    def set_solutions_packed(self, rec, met_size: int, field_sizes) -> None:
        """Packed per-vertex records (pack_solutions) in host or device memory
        (pmmg_hip_set_solutions_packed)."""
        where = DEVICE if _is_dev(rec) else HOST
        sizes = (ctypes.c_int * max(1, len(field_sizes)))(*[int(x) for x in field_sizes])
        self._sol_keep = [rec, sizes]
        self._ck(self.lib.pmmg_hip_set_solutions_packed(self.h, int(met_size), len(field_sizes), sizes, _p(rec),
                                                        where), "set_solutions_packed")

    def set_point_map(self, src) -> None:
        """pmmg_hip_set_point_map: arms the next locate_interp / locate_interp_rec
        with Mmg's point map — src[i] = 1-based background vertex new point i+1
        descends from (MMG5_Point.src under USE_POINTMAP), 0 = unknown.  A numpy
        array is copied; a device array must stay valid until the call is done."""
        if not _is_dev(src):
            src = np.ascontiguousarray(src, np.int32)
        elif np.dtype(src.dtype) != np.int32:
            raise ValueError("a device point map must be int32")
        self._map_keep = src
        self._ck(self.lib.pmmg_hip_set_point_map(self.h, int(src.shape[0]), _p(src),
                                                 DEVICE if _is_dev(src) else HOST), "set_point_map")

    def start_elements(self):
        """pmmg_hip_start_elements: (start_tet, start_tri) of the background as
        set, per vertex the lowest-index in-use tetra / boundary tria holding
        it (1-based, 0 = none): PMMG_locate_setStart's start elements."""
        npt = self._keep[0].shape[0]
        st, sr = np.zeros(npt, np.int32), np.zeros(npt, np.int32)
        self._ck(self.lib.pmmg_hip_start_elements(self.h, _p(st), _p(sr), HOST), "start_elements")
        return st, sr

    def locate_interp(self, xyz_new, pclass, met_out, fields_out, elem_out=None, hit_out=None,
                      sync: bool = True) -> HipStats | None:
        where = DEVICE if _is_dev(xyz_new) else HOST
        fields_out = list(fields_out)
        ptrs = (ctypes.c_void_p * max(1, len(fields_out)))(*[_p(f) for f in fields_out])
        st = HipStats()
        self._ck(self.lib.pmmg_hip_locate_interp(self.h, xyz_new.shape[0], _p(xyz_new), _p(pclass), _p(met_out),
                                                 ptrs, _p(elem_out), _p(hit_out),
                                                 ctypes.byref(st) if (sync or where == HOST) else None, where),
                 "locate_interp")
        return st if (sync or where == HOST) else None

    def locate_interp_rec(self, xyz_new, pclass, rec_out, elem_out=None, hit_out=None,
                          sync: bool = True) -> HipStats | None:
        """pmmg_hip_locate_interp_rec: device arrays; after set_solutions_packed,
        the new points' values as records of the packed layout (rec_out
        [np_new, RS])."""
        st = HipStats()
        self._ck(self.lib.pmmg_hip_locate_interp_rec(self.h, xyz_new.shape[0], _p(xyz_new), _p(pclass), _p(rec_out),
                                                     _p(elem_out), _p(hit_out), ctypes.byref(st) if sync else None,
                                                     DEVICE), "locate_interp_rec")
        return st if sync else None

    def locate_interp_groups(self, groups, sync: bool = True) -> HipStats | None:
        """pmmg_hip_locate_interp_groups: many groups in one call, device
        arrays only.  Each group is a dict {xyz, tet8 | (tetv, adja), triv,
        adjt, hausd, met, fields, xyz_new, pclass, met_out, fields_out[,
        elem_out, hit_out]}.  sync: wait and return the summed counters;
        otherwise only enqueue (pmmg_hip_sync before reading outputs)."""
        G = (HipGroup * max(1, len(groups)))()
        keep = []
        for i, g in enumerate(groups):
            arrays = [g["xyz"], g.get("tet8"), g.get("tetv"), g.get("adja"), g["triv"], g.get("adjt"), g.get("met"),
                      g["xyz_new"], g["pclass"], g.get("met_out"), g.get("elem_out"), g.get("hit_out")]
            arrays += list(g.get("fields", [])) + list(g.get("fields_out", []))
            if not all(a is None or _is_dev(a) for a in arrays):
                raise ValueError(f"group {i}: locate_interp_groups takes device arrays")
            fs, fo = list(g.get("fields", [])), list(g.get("fields_out", []))
            fsz = (ctypes.c_int * max(1, len(fs)))(*[int(f.shape[1]) for f in fs])
            fpt = (ctypes.c_void_p * max(1, len(fs)))(*[_p(f) for f in fs])
            opt = (ctypes.c_void_p * max(1, len(fo)))(*[_p(f) for f in fo])
            keep += [fsz, fpt, opt, arrays]
            tet = g["tet8"] if g.get("tet8") is not None else g["tetv"]
            met = g.get("met")
            v = lambda a: None if a is None else _p(a).value  # noqa: E731
            G[i] = HipGroup(int(g["xyz"].shape[0]), int(tet.shape[0]), int(g["triv"].shape[0]), v(g["xyz"]),
                            v(g.get("tet8")), v(g.get("tetv")), v(g.get("adja")), v(g["triv"]), v(g.get("adjt")),
                            float(g["hausd"]), 0 if met is None else int(met.shape[1]), v(met), len(fs),
                            ctypes.cast(fsz, ctypes.c_void_p), ctypes.cast(fpt, ctypes.c_void_p),
                            int(g["xyz_new"].shape[0]), v(g["xyz_new"]), v(g["pclass"]), v(g.get("met_out")),
                            ctypes.cast(opt, ctypes.c_void_p), v(g.get("elem_out")), v(g.get("hit_out")))
        self._grp_keep = (G, keep)
        st = HipStats()
        self._ck(self.lib.pmmg_hip_locate_interp_groups(self.h, len(groups), ctypes.cast(G, ctypes.c_void_p),
                                                        ctypes.byref(st) if sync else None), "locate_interp_groups")
        return st if sync else None

    def keep(self, slot: int = 0) -> None:
        """pmmg_hip_keep: the last host-mode call's new points and written rows
        stay on the device in `slot` (the next iteration's background)."""
        self._ck(self.lib.pmmg_hip_keep(self.h, int(slot)), "keep")

    def carry_over(self, slot: int, npt: int, src=None) -> None:
        """pmmg_hip_carry_over: the next host-mode set_background /
        set_solutions take vertex i+1 from kept point src[i] (1-based, 0: from
        the host arrays; None: the identity)."""
        s = None if src is None else np.ascontiguousarray(src, np.int32)
        self._ck(self.lib.pmmg_hip_carry_over(self.h, int(slot), int(npt), _p(s)), "carry_over")

    def release_scratch(self) -> None:
        """pmmg_hip_release_scratch: free the snapshot buckets, the binning's
        scratch, the reports' edge table, the element graph's, the contiguity calls' and the group split's
        scratch and the group lanes (re-allocated on demand)."""
        self._ck(self.lib.pmmg_hip_release_scratch(self.h), "release_scratch")

    def bytes_up(self, reset: bool = False) -> int:
        """host -> device bytes of host-mode calls (pmmg_hip_bytes_up)"""
        return int(self.lib.pmmg_hip_bytes_up(self.h, int(reset)))

    def tetra_qual(self, xyz, tetv, met=None, qual=None):
        """PMMG_tetraQual's MMG3D_tetraQual(mesh, met, 1) on the device
        (pmmg_hip_tetra_qual): device arrays (the metric where locate_interp
        wrote it).  Returns (qual DeviceArray [ne], ALPHAD * min quality)."""
        if not (_is_dev(xyz) and _is_dev(tetv) and (met is None or _is_dev(met))):
            raise ValueError("tetra_qual takes device arrays")
        ne = tetv.shape[0]
        qual = qual if qual is not None else self.empty((ne,), np.float64)
        mn = ctypes.c_double(0.0)
        self._ck(self.lib.pmmg_hip_tetra_qual(self.h, xyz.shape[0], _p(xyz), ne, _p(tetv),
                                              0 if met is None else int(met.shape[1]), _p(met), _p(qual),
                                              ctypes.byref(mn)), "tetra_qual")
        return qual, mn.value

    def qual_histo(self, tetv, qual) -> dict:
        """PMMG_qualhisto's per-group MMG3D_computeOutqua on the device
        (pmmg_hip_qual_histo): device arrays, qual as tetra_qual wrote it.
        Returns the struct as a dict (avg_sum is a sum: divide by ne_used)."""
        if not (_is_dev(tetv) and _is_dev(qual)):
            raise ValueError("qual_histo takes device arrays")
        out = HipQualHisto()
        self._ck(self.lib.pmmg_hip_qual_histo(self.h, tetv.shape[0], _p(tetv), _p(qual), ctypes.byref(out)),
                 "qual_histo")
        return out.as_dict()

    def edge_lengths(self, xyz, tetv, met, skip=None, want_edges=False, cap=None):
        """PMMG_computePrilen on the device (pmmg_hip_edge_lengths): device
        arrays (the metric where locate_interp wrote it, [np, 1] or [np, 6]);
        skip: device array [nskip, 2] of vertex-id pairs this rank must not
        analyse, or None.  Returns the struct as a dict, or with want_edges
        (dict, edges DeviceArray [n, 2], lengths DeviceArray [n]) in ascending
        (owner tetra, local edge) order, n = nedge - nskipped; cap: rows to
        allocate for the lists (None: one call without lists counts first)."""
        if not (_is_dev(xyz) and _is_dev(tetv) and _is_dev(met)) or (skip is not None and not _is_dev(skip)):
            raise ValueError("edge_lengths takes device arrays")
        nskip = 0 if skip is None else int(skip.shape[0])

        def call(cap_, edges, lens):
            out = HipLenHisto()
            ok = self.lib.pmmg_hip_edge_lengths(self.h, xyz.shape[0], _p(xyz), tetv.shape[0], _p(tetv),
                                                int(met.shape[1]), _p(met), nskip, _p(skip), ctypes.byref(out),
                                                int(cap_), _p(edges), _p(lens))
            self._ck(ok, "edge_lengths")
            return out

        if not want_edges:
            return call(0, None, None).as_dict()
        if cap is None:
            first = call(0, None, None)
            cap = first.nedge - first.nskipped
        edges, lens = self.empty((int(cap), 2), np.int32), self.empty((int(cap),), np.float64)
        out = call(cap, edges, lens)
        n = int(out.nedge - out.nskipped)
        edges.shape, edges.nbytes = (n, 2), n * 8
        lens.shape, lens.nbytes = (n,), n * 8
        return out.as_dict(), edges, lens

    def mesh_stats_bytes(self) -> int:
        """device bytes of the two reports' scratch (pmmg_hip_mesh_stats_bytes)"""
        return int(self.lib.pmmg_hip_mesh_stats_bytes(self.h))

    def compute_wgt_mesh(self, xyz, tetv, xt, ftag, met, tag, qual):
        """PMMG_computeWgt_mesh on the device (pmmg_hip_compute_wgt_mesh):
        device arrays; qual is updated in place for tetra with an xtetra."""
        if not all(_is_dev(a) for a in (xyz, tetv, xt, ftag, qual)) or (met is not None and not _is_dev(met)):
            raise ValueError("compute_wgt_mesh takes device arrays")
        self._ck(self.lib.pmmg_hip_compute_wgt_mesh(self.h, xyz.shape[0], _p(xyz), tetv.shape[0], _p(tetv), _p(xt),
                                                    _p(ftag), 0 if met is None else int(met.shape[1]), _p(met),
                                                    int(tag), _p(qual)), "compute_wgt_mesh")
        return qual

    def compute_wgt_faces(self, xyz, tetv, face, met, wgt=None):
        """PMMG_computeWgt of a (tetra, face) list (pmmg_hip_compute_wgt_faces)."""
        if not all(_is_dev(a) for a in (xyz, tetv, face)) or (met is not None and not _is_dev(met)):
            raise ValueError("compute_wgt_faces takes device arrays")
        nf = face.shape[0]
        wgt = wgt if wgt is not None else self.empty((nf,), np.float64)
        self._ck(self.lib.pmmg_hip_compute_wgt_faces(self.h, xyz.shape[0], _p(xyz), _p(tetv), nf, _p(face),
                                                     0 if met is None else int(met.shape[1]), _p(met), _p(wgt)),
                 "compute_wgt_faces")
        return wgt

    def metis_graph(self, xyz, tetv, adja=None, tet8=None, met=None, weights=True, cap=None, out=None):
        """PMMG_graph_meshElts2metis on the device (pmmg_hip_metis_graph):
        device arrays.  Tetra from tet8 ([ne, 8] packed records) when given,
        else from tetv + adja; with neither adja nor tet8 the adjacency is
        built on the device first.  weights=False: the unweighted graph (xyz
        and met are not read and may be None); weights without a metric are
        all PMMG_WGTVAL_HUGEINT.  Returns (xadj [ne + 1], adjncy [n], adjwgt
        [n] | None) DeviceArrays, n = xadj[ne]; cap: rows to allocate for the
        lists (None: 4 ne, one per face); out = (xadj, adjncy, adjwgt) arrays
        to fill instead of new ones."""
        given = [a for a in (xyz, tetv, adja, tet8, met) if a is not None]
        if not all(_is_dev(a) for a in given):
            raise ValueError("metis_graph takes device arrays")
        ne = (tet8 if tet8 is not None else tetv).shape[0]
        cap = 4 * ne if cap is None else int(cap)
        if out is not None:
            xadj, adjncy, adjwgt = out
        else:
            xadj = self.empty((ne + 1,), np.int32)
            adjncy = self.empty((cap,), np.int32)
            adjwgt = self.empty((cap,), np.int32) if weights else None
        n = ctypes.c_int64(0)
        self._ck(self.lib.pmmg_hip_metis_graph(self.h, 0 if xyz is None else xyz.shape[0], _p(xyz), ne, _p(tetv),
                                               _p(adja), _p(tet8), 0 if met is None else int(met.shape[1]), _p(met),
                                               cap, ctypes.byref(n), _p(xadj), _p(adjncy),
                                               _p(adjwgt) if weights else None), "metis_graph")
        if out is None:
            for a in (adjncy, adjwgt):
                if a is not None:
                    a.shape, a.nbytes = (n.value,), 4 * n.value
        return xadj, adjncy, (adjwgt if weights else None)

    def part_subgroups(self, tetv, adja=None, tet8=None, part=None, ncolor=1, head=None, flag=None, cap=None):
        """The subgroups (connected components of the adjacency restricted to
        one colour) of a partition on the device (pmmg_hip_part_subgroups):
        device arrays.  Tetra from tet8 when given, else from adja; tetv may
        be None when adja is given; with neither adja nor tet8 the adjacency is
        built on the device.  part [ne] in [0, ncolor), or None: one colour.
        head / flag: int32 device arrays [ne] to fill, or None.  Returns
        dict(ncomp [ncolor], sub [nsub, 4] = color, head, size, exit in
        ascending head, rounds, passes); cap: rows of the table (None: one
        call counts first)."""
        given = [a for a in (tetv, adja, tet8, part, head, flag) if a is not None]
        if not all(_is_dev(a) for a in given):
            raise ValueError("part_subgroups takes device arrays")
        ne = (tet8 if tet8 is not None else (adja if adja is not None else tetv)).shape[0]
        ncomp = (ctypes.c_int * int(ncolor))()
        n, rounds = ctypes.c_int64(0), ctypes.c_int(0)

        def call(cap_, table):
            return self.lib.pmmg_hip_part_subgroups(self.h, ne, _p(tetv), _p(adja), _p(tet8), _p(part), int(ncolor),
                                                    _p(head), _p(flag), ncomp, int(cap_), table, ctypes.byref(n),
                                                    ctypes.byref(rounds))

        if cap is None:
            if not call(0, None) and n.value == 0:
                self._ck(0, "part_subgroups")
            cap = n.value
        table = (HipSubgroup * max(1, int(cap)))()
        self._ck(call(cap, table), "part_subgroups")
        sub = np.array([(r.color, r.head, r.size, r.exit) for r in table[:n.value]], np.int32).reshape(-1, 4)
        return dict(ncomp=np.array(list(ncomp), np.int32), sub=sub, rounds=rounds.value,
                    passes=int(self.lib.pmmg_hip_contig_passes(self.h)))

    def fix_contiguity(self, tetv, part, ncolor, adja=None, tet8=None):
        """PMMG_fix_contiguity for colours 0 .. ncolor-1 on the device
        (pmmg_hip_fix_contiguity): part (device int32 [ne]) is changed in
        place.  Returns dict(nmoved, nmerged, nstuck, passes)."""
        given = [a for a in (tetv, adja, tet8, part) if a is not None]
        if not all(_is_dev(a) for a in given):
            raise ValueError("fix_contiguity takes device arrays")
        ne = (tet8 if tet8 is not None else (adja if adja is not None else tetv)).shape[0]
        nmoved, nmerged, nstuck = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int(0)
        self._ck(self.lib.pmmg_hip_fix_contiguity(self.h, ne, _p(tetv), _p(adja), _p(tet8), _p(part), int(ncolor),
                                                  ctypes.byref(nmoved), ctypes.byref(nmerged), ctypes.byref(nstuck)),
                 "fix_contiguity")
        return dict(nmoved=nmoved.value, nmerged=nmerged.value, nstuck=nstuck.value,
                    passes=int(self.lib.pmmg_hip_contig_passes(self.h)))

    # ------------------------------------------------------------------ interface displacement
    def interface_points(self, npt, mark, weight, tetv=None, tet8=None):
        """PMMG_mark_interfacePoints on the device (pmmg_hip_ifc_seed): tetv or
        tet8 and mark [ne] are device arrays, weight [ncolor] a host array (c
        beats d iff weight[c] < weight[d]).  Returns (ptcolor int32 [np],
        ptfront uint8 [np]) as DeviceArrays."""
        if not all(_is_dev(a) for a in (tetv, tet8, mark) if a is not None):
            raise ValueError("interface_points takes device arrays")
        weight = np.ascontiguousarray(weight, np.int32)
        ne = int((tet8 if tet8 is not None else tetv).shape[0])
        color, front = self.empty((int(npt),), np.int32), self.empty((int(npt),), np.uint8)
        self._ck(self.lib.pmmg_hip_ifc_seed(self.h, int(npt), ne, _p(tetv), _p(tet8), _p(mark), weight.size, _p(weight),
                                            _p(color), _p(front)), "ifc_seed")
        return color, front

    def move_interfaces(self, npt, mark, weight, nelem, tetv=None, tet8=None, adja=None, ptcolor=None, ptfront=None,
                        nlayers=2, set_pt=None, set_color=None, nemin=None, fix=True):
        """The layer loop of PMMG_part_moveInterfaces on the device
        (pmmg_hip_ifc_layers), then PMMG_fix_contiguity when fix is true and no
        layer was blocked.  mark (device int32 [ne]) is changed in place.
        weight, nelem (-1: a colour of another rank) are host arrays [ncolor];
        nemin None: the reference's MG_MIN(6, nelem / 2 + 1).  ptcolor /
        ptfront: the state of interface_points or of an earlier call, changed
        in place (None: seeded here).  set_pt / set_color: device int32 arrays
        of points made front before every layer and their colours before the
        first.  Returns dict(layers_done, blocked, moved [nlayers], nelem,
        ptcolor, ptfront, fix = fix_contiguity's dict or None)."""
        given = [a for a in (tetv, tet8, adja, mark, ptcolor, ptfront, set_pt, set_color) if a is not None]
        if not all(_is_dev(a) for a in given):
            raise ValueError("move_interfaces takes device arrays")
        weight = np.ascontiguousarray(weight, np.int32)
        nelem = np.array(nelem, np.int32)
        if nemin is None:
            nemin = np.where(nelem >= 0, np.minimum(6, nelem // 2 + 1), 0)
        nemin = np.ascontiguousarray(nemin, np.int32)
        if ptcolor is None:
            ptcolor, ptfront = self.interface_points(npt, mark, weight, tetv=tetv, tet8=tet8)
        ne = int((tet8 if tet8 is not None else tetv).shape[0])
        nset = 0 if set_pt is None else int(set_pt.shape[0])
        moved = np.zeros(max(1, int(nlayers)), np.int32)
        done, blocked = ctypes.c_int(0), ctypes.c_int(0)
        self._ck(self.lib.pmmg_hip_ifc_layers(self.h, int(npt), ne, _p(tetv), _p(tet8), _p(mark), weight.size, _p(weight),
                                              _p(nelem), _p(nemin), _p(ptcolor), _p(ptfront), nset, _p(set_pt),
                                              _p(set_color), int(nlayers), ctypes.byref(done), ctypes.byref(blocked),
                                              _p(moved)), "ifc_layers")
        fixed = None
        if fix and not blocked.value:
            fixed = self.fix_contiguity(tetv, mark, weight.size, adja=adja, tet8=tet8)
        return dict(layers_done=done.value, blocked=blocked.value, moved=moved[:int(nlayers)], nelem=nelem,
                    ptcolor=ptcolor, ptfront=ptfront, fix=fixed)

    def remap_colors(self, mark, ncolor, order=None, tetv=None, tet8=None, part=None):
        """The packing of PMMG_part_getInterfaces (pmmg_hip_remap_colors): the
        colours present among the used tetra numbered 0, 1, ... in ascending
        order[colour] (None: the colours' own order).  Returns (part, ngrp);
        part: the device array to fill, or None for a new one."""
        if not all(_is_dev(a) for a in (tetv, tet8, mark, part) if a is not None):
            raise ValueError("remap_colors takes device arrays")
        order = np.ascontiguousarray(np.arange(int(ncolor)) if order is None else order, np.int32)
        ne = int((tet8 if tet8 is not None else tetv).shape[0])
        part = self.empty((ne,), np.int32) if part is None else part
        ngrp = ctypes.c_int(0)
        self._ck(self.lib.pmmg_hip_remap_colors(self.h, ne, _p(tetv), _p(tet8), _p(mark), int(ncolor), _p(order),
                                                _p(part), ctypes.byref(ngrp)), "remap_colors")
        return part, ngrp.value

    # ------------------------------------------------------------------ group split
    def split_groups(self, npt, part, ngrp, tetv=None, adja=None, tet8=None, node_pos=None, face_old=None, nnode0=0,
                     nface0=0, caps=None, want=("new_tet", "tet8_out")):
        """PMMG_split_grps on the device (pmmg_hip_split_groups): device
        arrays in, device arrays out.  Tetra from tet8 when given, else from
        tetv + adja; part [ne] in [0, ngrp).  want: which of new_tet, tetv_out,
        adja_out, tet8_out to write.  caps = (pt_cap, face_cap, node_cap), or
        None: a first call with caps of 0 sizes the lists.  Returns a dict:
        count [ngrp, 4] = ne, np, nface, nnode per group (host), the offset
        tables te_off, pt_off, face_off, node_off [ngrp + 1] (host, exclusive
        prefix sums of the counts), old_tet and the arrays of `want` [ne], old_pt,
        face_idx1, face_idx2, node_idx1, node_idx2 (DeviceArrays of exactly
        the lists' lengths, groups concatenated), nnode_end, nface_end,
        rounds."""
        given = [a for a in (tetv, adja, tet8, part, node_pos, face_old) if a is not None]
        if not all(_is_dev(a) for a in given):
            raise ValueError("split_groups takes device arrays")
        unknown = set(want) - {"new_tet", "tetv_out", "adja_out", "tet8_out"}
        if unknown:
            raise ValueError(f"split_groups: unknown outputs {sorted(unknown)}")
        ne, ngrp = int((tet8 if tet8 is not None else tetv).shape[0]), int(ngrp)
        count = (HipSplitCount * max(1, ngrp))()
        nn, nf = ctypes.c_int(0), ctypes.c_int(0)
        out = dict(old_tet=self.empty((ne,), np.int32))
        for k, cols in (("new_tet", None), ("tetv_out", 4), ("adja_out", 4), ("tet8_out", 8)):
            out[k] = self.empty((ne,) if cols is None else (ne, cols), np.int32) if k in want else None

        def call(caps_, lists):
            return self.lib.pmmg_hip_split_groups(
                self.h, int(npt), ne, _p(tetv), _p(adja), _p(tet8), _p(part), ngrp, _p(node_pos), _p(face_old),
                int(nnode0), int(nface0), count, int(caps_[0]), int(caps_[1]), int(caps_[2]), _p(out["old_tet"]),
                _p(out["new_tet"]), _p(out["tetv_out"]), _p(out["adja_out"]), _p(out["tet8_out"]), *[_p(a) for a in lists],
                ctypes.byref(nn), ctypes.byref(nf))

        def totals():
            c = np.array([(r.ne, r.np, r.nface, r.nnode) for r in count[:ngrp]], np.int64).reshape(-1, 4)
            return c, [int(x) for x in c.sum(axis=0)]

        try:
            if caps is None:
                if not call((0, 0, 0), [None] * 5):
                    c, tot = totals()
                    if tot[0] != ne:  # (a refusal, not a cap: the counts were not filled)
                        self._ck(0, "split_groups")
                    caps = tot[1:]
                else:
                    caps = (0, 0, 0)
            lists = [self.empty((int(caps[0]),), np.int32)] + [self.empty((int(caps[1]),), np.int32) for _ in range(2)]
            lists += [self.empty((int(caps[2]),), np.int32) for _ in range(2)]
            try:
                self._ck(call(caps, lists), "split_groups")
            except Exception:
                _free_all(lists)
                raise
        except Exception:
            _free_all(out.values())
            raise
        c, tot = totals()
        for a, n in zip(lists, (tot[1], tot[2], tot[2], tot[3], tot[3])):  # (a cap may exceed its list)
            a.shape, a.nbytes = (n,), 4 * n
        off = np.concatenate([np.zeros((1, 4), np.int64), np.cumsum(c, axis=0)])
        out.update(count=c.astype(np.int32), te_off=off[:, 0], pt_off=off[:, 1], face_off=off[:, 2], node_off=off[:, 3],
                   old_pt=lists[0], face_idx1=lists[1], face_idx2=lists[2], node_idx1=lists[3], node_idx2=lists[4],
                   nnode_end=nn.value, nface_end=nf.value, rounds=int(self.lib.pmmg_hip_split_rounds(self.h)))
        return out

    def gather_rows(self, src, rows, out=None):
        """out row r = rows row src[r] - 1 on the device (pmmg_hip_gather_rows):
        src int32 [n] 1-based, rows float64 [m, size].  Returns the DeviceArray
        [n, size] (out, when given)."""
        return self._gather("gather_rows", np.float64, src, rows, out)

    def _gather(self, name, dtype, src, rows, out):
        """gather_rows and gather_rows_i32: pmmg_hip_<name> on rows [m] or [m, size] of dtype"""
        if not (_is_dev(src) and _is_dev(rows) and (out is None or _is_dev(out))):
            raise ValueError(f"{name} takes device arrays")
        n, size = int(src.shape[0]), int(rows.shape[1]) if len(rows.shape) > 1 else 1
        if out is None:
            out = self.empty((n,) + tuple(rows.shape[1:]), dtype)
        self._ck(getattr(self.lib, "pmmg_hip_" + name)(self.h, n, _p(src), size, _p(rows), _p(out)), name)
        return out

    def groups_from_split(self, split, xyz, met=None, fields=()):
        """The background part of every group's pmmg_hip_group record from a
        split: a list of dicts {np, ne, xyz, tet8 | (tetv, adja), met, fields},
        whose arrays are views into `split`'s arrays and into the rows
        gathered here through old_pt (xyz, the metric, every field; device
        arrays [np_old, size]).  Complete each dict with triv / adjt / hausd
        and the new points, then pass the list to locate_interp_groups: nothing
        goes through the host.  The views own no memory: free the returned
        "owned" arrays and the split's, not the groups'."""
        old_pt = split["old_pt"]
        g_xyz = self.gather_rows(old_pt, xyz)
        g_met = None if met is None else self.gather_rows(old_pt, met)
        g_f = [self.gather_rows(old_pt, f) for f in fields]

        def view(a, lo, hi):
            row = a.nbytes // max(1, a.shape[0])
            return DeviceArray(a.ptr + int(lo) * row, int(hi - lo) * row, (int(hi - lo),) + tuple(a.shape[1:]), a.dtype,
                               self)

        groups = []
        for g in range(split["count"].shape[0]):
            t0, t1, p0, p1 = split["te_off"][g], split["te_off"][g + 1], split["pt_off"][g], split["pt_off"][g + 1]
            d = dict(np=int(p1 - p0), ne=int(t1 - t0), xyz=view(g_xyz, p0, p1), met=None if g_met is None else view(g_met, p0, p1),
                     fields=[view(f, p0, p1) for f in g_f])
            if split.get("tet8_out") is not None:
                d["tet8"] = view(split["tet8_out"], t0, t1)
            else:
                d["tetv"], d["adja"] = view(split["tetv_out"], t0, t1), view(split["adja_out"], t0, t1)
            groups.append(d)
        return groups, [g_xyz] + ([] if g_met is None else [g_met]) + g_f

    # ------------------------------------------------------------------ group merge
    def merge_groups(self, split_or_arrays, color=None, nnode=None, nface=None, pt_cap=None,
                     want=("new_tet", "tetv_out", "node_val", "face_val")):
        """PMMG_merge_grps steps 0-4 on the device (pmmg_hip_merge_groups):
        device arrays in, device arrays out.  split_or_arrays: the dict that
        split_groups returns, or one with count [ngrp, 4] (host), tet8_out or
        tetv_out, face_idx1, face_idx2, node_idx1, node_idx2 (device, groups
        concatenated), and nnode_end / nface_end unless nnode / nface (the two
        nitem) are given.  color [ngrp] (host) or None: the mark of every
        group's tetra (mark_out).  want: which of new_tet, tetv_out, node_val,
        face_val to write.  pt_cap None: the groups' points, which the merged
        points never exceed.  Returns a dict: np, ne, new_pt [sum np], src_pt
        [np], src_tet [ne], mark_out (with color) and the arrays of `want`."""
        a = split_or_arrays
        unknown = set(want) - {"new_tet", "tetv_out", "node_val", "face_val"}
        if unknown:
            raise ValueError(f"merge_groups: unknown outputs {sorted(unknown)}")
        tet8, tetv = a.get("tet8_out"), a.get("tetv_out")
        if tet8 is not None:
            tetv = None
        lists = [a["node_idx1"], a["node_idx2"], a["face_idx1"], a["face_idx2"]]
        if not all(_is_dev(x) for x in lists + [tet8, tetv] if x is not None):
            raise ValueError("merge_groups takes device arrays")
        c = np.ascontiguousarray(a["count"], np.int32).reshape(-1, 4)
        ngrp = int(c.shape[0])
        count = (HipSplitCount * max(1, ngrp))(*[HipSplitCount(*[int(v) for v in r]) for r in c])
        tne, tnp = int(c[:, 0].sum()), int(c[:, 1].sum())
        nnode = int(a["nnode_end"] if nnode is None else nnode)
        nface = int(a["nface_end"] if nface is None else nface)
        cap = tnp if pt_cap is None else int(pt_cap)
        color = None if color is None else np.ascontiguousarray(color, np.int32)
        if color is not None and color.shape != (ngrp,):
            raise ValueError("merge_groups: color must hold one entry per group")
        out = dict(new_pt=self.empty((tnp,), np.int32), src_pt=self.empty((cap,), np.int32),
                   src_tet=self.empty((tne,), np.int32),
                   new_tet=self.empty((tne,), np.int32) if "new_tet" in want else None,
                   tetv_out=self.empty((tne, 4), np.int32) if "tetv_out" in want else None,
                   mark_out=self.empty((tne,), np.int32) if color is not None else None,
                   node_val=self.empty((nnode,), np.int32) if "node_val" in want else None,
                   face_val=self.empty((nface,), np.int32) if "face_val" in want else None)
        npo, neo = ctypes.c_int(0), ctypes.c_int(0)
        ok = self.lib.pmmg_hip_merge_groups(
            self.h, ngrp, count, _p(tetv), _p(tet8), *[_p(x) for x in lists], nnode, nface, _p(color), cap,
            _p(out["new_pt"]), _p(out["new_tet"]), _p(out["src_pt"]), _p(out["src_tet"]), _p(out["tetv_out"]),
            _p(out["mark_out"]), _p(out["node_val"]), _p(out["face_val"]), ctypes.byref(npo), ctypes.byref(neo))
        if not ok:
            _free_all(out.values())
            err = RuntimeError(f"merge_groups failed: {self.error()}")
            err.np, err.ne = npo.value, neo.value  # (filled when only pt_cap was short)
            raise err
        out["src_pt"].shape, out["src_pt"].nbytes = (npo.value,), 4 * npo.value  # (the cap may exceed the points)
        out.update(np=npo.value, ne=neo.value)
        return out

    def gather_rows_i32(self, src, rows, out=None):
        """gather_rows for int32 rows (pmmg_hip_gather_rows_i32): the ref /
        mark rows of the merged tetra through src_tet.  rows int32 [m] or
        [m, size]; returns the DeviceArray [n] or [n, size] (out, when given)."""
        return self._gather("gather_rows_i32", np.int32, src, rows, out)

    def merged_from_groups(self, merge, xyz, met=None, fields=()):
        """The point rows of the merged mesh from the groups' (device arrays
        [sum np, size], groups concatenated, as groups_from_split's "owned"
        arrays are): gathered through merge["src_pt"] with gather_rows.  Returns
        (xyz, met or None, [fields]) of merge["np"] rows each."""
        src = merge["src_pt"]
        return (self.gather_rows(src, xyz), None if met is None else self.gather_rows(src, met),
                [self.gather_rows(src, f) for f in fields])

    # ------------------------------------------------------------------ split over GPUs (RCCL)
    @staticmethod
    def comm_unique_id() -> bytes:
        """pmmg_hip_comm_unique_id: the RCCL id one rank makes and broadcasts."""
        buf = ctypes.create_string_buffer(128)
        if not hip_lib().pmmg_hip_comm_unique_id(buf):
            raise RuntimeError("pmmg_hip_comm_unique_id failed (RCCL unavailable?)")
        return buf.raw

    def comm_init(self, nranks: int, rank: int, uid: bytes) -> None:
        """pmmg_hip_comm_init (collective over the nranks processes)."""
        buf = ctypes.create_string_buffer(bytes(uid), 128)
        self._ck(self.lib.pmmg_hip_comm_init(self.h, int(nranks), int(rank), buf), "comm_init")

    def allgather_points(self, counts, rows, rows_all, elem=None, elem_all=None, hit=None, hit_all=None) -> None:
        """pmmg_hip_allgather_points: this rank's rows (device arrays / tensors,
        one per slot) and optional elem / hit gathered in rank order into
        rows_all / elem_all / hit_all on every rank."""
        cnt = np.ascontiguousarray(counts, np.int64)
        rows, rows_all = list(rows), list(rows_all)
        sizes = (ctypes.c_int * max(1, len(rows)))(*[int(r.shape[1]) for r in rows])
        rin = (ctypes.c_void_p * max(1, len(rows)))(*[_p(r) for r in rows])
        rout = (ctypes.c_void_p * max(1, len(rows_all)))(*[_p(r) for r in rows_all])
        self._ck(self.lib.pmmg_hip_allgather_points(self.h, _p(cnt), len(rows), sizes, rin, rout, _p(elem),
                                                    _p(elem_all), _p(hit), _p(hit_all)), "allgather_points")

    def sync(self) -> HipStats:
        st = HipStats()
        self._ck(self.lib.pmmg_hip_sync(self.h, ctypes.byref(st)), "sync")
        return st


def transfer(mesh_old, met, fields, xyz_new, pclass, hausd=0.01, device=0, sort=None, ctx=None):
    """One-shot host-mode transfer: returns (met_new, fields_new, elem, hit, stats)."""
    own = ctx is None
    ctx = ctx or TransferContext(device, sort=sort)
    try:
        ctx.set_background(mesh_old.xyz, mesh_old.tetv, mesh_old.adja, mesh_old.triv, mesh_old.adjt, hausd)
        ctx.set_solutions(met, fields)
        npn = xyz_new.shape[0]
        met_out = None if met is None else np.zeros((npn, met.shape[1]))
        f_out = [np.zeros((npn, f.shape[1])) for f in fields]
        elem = np.zeros(npn, np.int32)
        hit = np.zeros(npn, np.int8)
        st = ctx.locate_interp(np.ascontiguousarray(xyz_new), np.ascontiguousarray(pclass), met_out, f_out, elem, hit)
        return met_out, f_out, elem, hit, st
    finally:
        if own:
            ctx.close()


# ---------------------------------------------------------------- C host layer (csrc/pmmg_host.h)

class OldGroup(ctypes.Structure):
    _fields_ = [("np", ctypes.c_int), ("ne", ctypes.c_int), ("nt", ctypes.c_int),
                ("xyz", ctypes.c_void_p), ("tag", ctypes.c_void_p), ("tetv", ctypes.c_void_p),
                ("adja", ctypes.c_void_p), ("triv", ctypes.c_void_p), ("adjt", ctypes.c_void_p),
                ("hausd", ctypes.c_double), ("met_size", ctypes.c_int), ("met", ctypes.c_void_p),
                ("nfield", ctypes.c_int), ("field_size", ctypes.c_void_p), ("field", ctypes.c_void_p)]


class NewGroup(ctypes.Structure):
    _fields_ = [("np", ctypes.c_int), ("ne", ctypes.c_int), ("xyz", ctypes.c_void_p), ("tag", ctypes.c_void_p),
                ("tetv", ctypes.c_void_p), ("met_size", ctypes.c_int), ("met", ctypes.c_void_p),
                ("field", ctypes.c_void_p), ("elem", ctypes.c_void_p), ("hit", ctypes.c_void_p),
                ("hsiz", ctypes.c_double), ("hmin", ctypes.c_double), ("hmax", ctypes.c_double),
                ("ani", ctypes.c_int)]


TAG_REQ, TAG_BDY, TAG_NUL = 1 << 2, 1 << 4, 1 << 14


class _Groups:
    """ctypes views of old/new group dicts (keeps every array alive).

    old: {mesh, met, fields, hausd[, tag, device_adjacency, device_boundary]}
    new: {xyz, tag, tetv, met, fields[, elem, hit, hsiz, hmin, hmax, ani]}"""

    def __init__(self, old_groups, new_groups):
        ng = len(old_groups)
        self.olds = (OldGroup * ng)()
        self.news = (NewGroup * ng)()
        self.keep = []
        for i, (o, g) in enumerate(zip(old_groups, new_groups)):
            m = o["mesh"]
            fs = list(o.get("fields", []))
            fsz = (ctypes.c_int * max(1, len(fs)))(*[f.shape[1] for f in fs])
            fpt = (ctypes.c_void_p * max(1, len(fs)))(*[_p(f) for f in fs])
            met = o.get("met")
            dev_bdy = o.get("device_boundary", False)
            self.olds[i] = OldGroup(m.np, m.ne, -1 if dev_bdy else m.nt, _p(m.xyz), _p(o.get("tag")), _p(m.tetv),
                                    None if o.get("device_adjacency", False) else _p(m.adja),
                                    None if dev_bdy else _p(m.triv), None if dev_bdy else _p(m.adjt),
                                    float(o.get("hausd", 0.01)), 0 if met is None else met.shape[1], _p(met),
                                    len(fs), ctypes.cast(fsz, ctypes.c_void_p), ctypes.cast(fpt, ctypes.c_void_p))
            gf = list(g.get("fields", []))
            gpt = (ctypes.c_void_p * max(1, len(gf)))(*[_p(f) for f in gf])
            gm = g.get("met")
            self.news[i] = NewGroup(g["xyz"].shape[0], g["tetv"].shape[0], _p(g["xyz"]), _p(g.get("tag")),
                                    _p(g["tetv"]), 0 if gm is None else gm.shape[1], _p(gm),
                                    ctypes.cast(gpt, ctypes.c_void_p), _p(g.get("elem")), _p(g.get("hit")),
                                    float(g.get("hsiz", 0.0)), float(g.get("hmin", 0.0)), float(g.get("hmax", 0.0)),
                                    int(g.get("ani", 0)))
            self.keep += [fsz, fpt, gpt]


def interp_metrics_and_fields(ctx: TransferContext, old_groups, new_groups, input_met: int = 1, carry=None,
                              src=None):
    """PMMG_interpMetricsAndFields over groups (src/interpmesh_pmmg.c:663-741)
    through the C host layer (pmmg_interp_metrics_and_fields).  The new
    groups' ``met`` / ``fields`` arrays are filled in place; per-group
    ``hsiz`` > 0 replaces the metric by a constant (MMG3D_Set_constantSize).
    carry: None (plain call), or (carried, src) for
    pmmg_interp_metrics_and_fields_carry — the new groups stay on the device,
    and with carried the old groups are the previous call's new groups (src:
    None, or per group None / the 1-based map of its vertices onto them).
    src: per group None / Mmg's point map of its new points (MMG5_Point.src,
    1-based old-group vertex, 0 = unknown) for
    pmmg_interp_metrics_and_fields_map; not together with carry.
    Returns (ier, stats)."""
    G = _Groups(old_groups, new_groups)
    st = HipStats()
    if src is not None:
        if carry is not None:
            raise ValueError("interp_metrics_and_fields: src= and carry= are separate entry points")
        arrs = [None if m is None else np.ascontiguousarray(m, np.int32) for m in src]
        maps = (ctypes.c_void_p * max(1, len(arrs)))(*[None if a is None else _p(a).value for a in arrs])
        G.keep.append(arrs)
        ier = host_lib().pmmg_interp_metrics_and_fields_map(ctx.h, len(old_groups),
                                                            ctypes.cast(G.olds, ctypes.c_void_p),
                                                            ctypes.cast(G.news, ctypes.c_void_p), int(input_met),
                                                            ctypes.cast(maps, ctypes.c_void_p), ctypes.byref(st))
        return ier, st
    if carry is None:
        ier = host_lib().pmmg_interp_metrics_and_fields(ctx.h, len(old_groups), ctypes.cast(G.olds, ctypes.c_void_p),
                                                        ctypes.cast(G.news, ctypes.c_void_p), int(input_met),
                                                        ctypes.byref(st))
        return ier, st
    carried, src = carry
    maps = None
    if src is not None:
        arrs = [None if m is None else np.ascontiguousarray(m, np.int32) for m in src]
        maps = (ctypes.c_void_p * max(1, len(arrs)))(*[None if a is None else _p(a).value for a in arrs])
        G.keep.append(arrs)
    ier = host_lib().pmmg_interp_metrics_and_fields_carry(ctx.h, len(old_groups), ctypes.cast(G.olds, ctypes.c_void_p),
                                                          ctypes.cast(G.news, ctypes.c_void_p), int(input_met),
                                                          int(bool(carried)),
                                                          None if maps is None else ctypes.cast(maps, ctypes.c_void_p),
                                                          ctypes.byref(st))
    return ier, st


def copy_metrics_and_fields_point(old_group, new_group, perm_nod_glob=None, renum: int = 1, input_met: int = 1):
    """PMMG_copyMetricsAndFields_point (src/interpmesh_pmmg.c:432-446) through
    the C host layer: rows of the old group's valid MG_REQ points copied into
    the new group's arrays (through perm_nod_glob, 1-based with entry 0
    unused, when renum and a permutation are given).  Returns 1/0."""
    G = _Groups([old_group], [new_group])
    perm = None if perm_nod_glob is None else np.ascontiguousarray(perm_nod_glob, np.int32)
    return host_lib().pmmg_copy_metrics_and_fields_point(ctypes.cast(G.olds, ctypes.c_void_p),
                                                         ctypes.cast(G.news, ctypes.c_void_p), _p(perm),
                                                         int(renum), int(input_met))


def classify_points(new_group) -> np.ndarray:
    """The reference's point classification (src/interpmesh_pmmg.c:535-550)
    through the C host layer: PT_SKIP / PT_VOL / PT_BDY per new point."""
    g = dict(new_group)
    g.setdefault("fields", [])
    G = _Groups([dict(mesh=_EmptyMesh(), fields=[])], [g])
    pc = np.empty(g["xyz"].shape[0], np.uint8)
    host_lib().pmmg_classify_points(ctypes.cast(G.news, ctypes.c_void_p), _p(pc))
    return pc


def set_constant_metric(new_group) -> int:
    """MMG3D_Set_constantSize's fill through the C host layer (restated, unpinned)."""
    G = _Groups([dict(mesh=_EmptyMesh(), fields=[])], [new_group])
    return host_lib().pmmg_set_constant_metric(ctypes.cast(G.news, ctypes.c_void_p))


class _EmptyMesh:
    np = ne = nt = 0
    xyz = tetv = adja = triv = adjt = None
