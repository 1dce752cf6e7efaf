"""ctypes bindings of the native libraries.

The product path is ``libpmmg_hip.so`` (include/parmmg_hip.h) and the C host
layer ``libpmmg_host.so``.  Loading fails loudly when a library is missing:
there is no Python or CPU fallback for the transfer step.
"""
from __future__ import annotations

import ctypes
import os

from . import build as _build

c_int, c_int64, c_double, c_void_p, c_char_p = ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p, ctypes.c_char_p
P = ctypes.POINTER


ABI_VERSION = 6  # PMMG_HIP_ABI_VERSION of include/parmmg_hip.h


class HipStats(ctypes.Structure):
    """``pmmg_hip_stats`` of include/parmmg_hip.h."""

    _fields_ = [
        ("nvol", c_int64), ("nbdy", c_int64),
        ("nvol_walk", c_int64), ("nvol_exhaust", c_int64), ("nvol_closest", c_int64), ("nvol_exact", c_int64),
        ("nbdy_face", c_int64), ("nbdy_edge", c_int64), ("nbdy_vertex", c_int64), ("nbdy_wedge", c_int64),
        ("nbdy_cone", c_int64), ("nbdy_exhaust", c_int64), ("nbdy_stale", c_int64), ("nbdy_closest", c_int64),
        ("steps_total", c_int64), ("stepmax", c_int64), ("wave_iters", c_int64), ("sorted", c_int64),
        ("ms_prepare", ctypes.c_float), ("ms_sort", ctypes.c_float), ("ms_vol", ctypes.c_float),
        ("ms_bdy", ctypes.c_float), ("ms_fallback", ctypes.c_float), ("ms_total", ctypes.c_float),
        ("ms_vol_locate", ctypes.c_float),
        ("nvol_noseed", c_int64), ("nvol_stuck", c_int64), ("nvol_limit", c_int64), ("seed_map_axes", c_int64),
        ("nbdy_fanscan", c_int64), ("nvol_src", c_int64), ("nbdy_src", c_int64), ("reserved", c_int64 * 4),
    ]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class HipQualHisto(ctypes.Structure):
    """``pmmg_hip_qual_histo_t`` of include/parmmg_hip.h."""

    _fields_ = [
        ("ne_used", c_int64), ("max", c_double), ("min", c_double), ("iel", c_int64), ("avg_sum", c_double),
        ("good", c_int64), ("med", c_int64), ("his", c_int64 * 5), ("reserved", c_int64 * 4),
    ]

    def as_dict(self) -> dict:
        d = {name: getattr(self, name) for name, _ in self._fields_ if name not in ("his", "reserved")}
        d["his"] = list(self.his)
        return d


class HipLenHisto(ctypes.Structure):
    """``pmmg_hip_len_histo_t`` of include/parmmg_hip.h."""

    _fields_ = [
        ("nedge", c_int64), ("nskipped", c_int64), ("ned", c_int64), ("nnull", c_int64), ("avlen_sum", c_double),
        ("lmin", c_double), ("lmax", c_double), ("amin", ctypes.c_int32), ("bmin", ctypes.c_int32),
        ("amax", ctypes.c_int32), ("bmax", ctypes.c_int32), ("hl", c_int64 * 9), ("reserved", c_int64 * 4),
    ]

    def as_dict(self) -> dict:
        d = {name: getattr(self, name) for name, _ in self._fields_ if name not in ("hl", "reserved")}
        d["hl"] = list(self.hl)
        return d


class HipSubgroup(ctypes.Structure):
    """``pmmg_hip_subgroup`` of include/parmmg_hip.h."""

    _fields_ = [("color", c_int), ("head", c_int), ("size", c_int), ("exit", c_int)]


class HipSplitCount(ctypes.Structure):
    """``pmmg_hip_split_count`` of include/parmmg_hip.h."""

    _fields_ = [("ne", c_int), ("np", c_int), ("nface", c_int), ("nnode", c_int)]


class HostSplitResult(ctypes.Structure):
    """``pmmg_split_result`` of csrc/pmmg_host.h."""

    _fields_ = [
        ("count", P(HipSplitCount)), ("npt", c_int64), ("nface", c_int64), ("nnode", c_int64),
        ("old_tet", P(c_int)), ("new_tet", P(c_int)), ("tetv", P(c_int)), ("adja", P(c_int)), ("old_pt", P(c_int)),
        ("xyz", P(c_double)), ("met", P(c_double)), ("met_size", c_int), ("nfield", c_int), ("fields", P(P(c_double))),
        ("face_idx1", P(c_int)), ("face_idx2", P(c_int)), ("node_idx1", P(c_int)), ("node_idx2", P(c_int)),
        ("nnode_end", c_int), ("nface_end", c_int),
    ]


class HostMergeResult(ctypes.Structure):
    """``pmmg_merge_result`` of csrc/pmmg_host.h."""

    _fields_ = [
        ("np", c_int), ("ne", c_int), ("new_pt", P(c_int)), ("src_pt", P(c_int)), ("new_tet", P(c_int)),
        ("src_tet", P(c_int)), ("tetv", P(c_int)), ("mark", P(c_int)), ("tref", P(c_int)), ("xyz", P(c_double)),
        ("met", P(c_double)), ("met_size", c_int), ("node_val", P(c_int)), ("face_val", P(c_int)),
    ]


class HipGroup(ctypes.Structure):
    """``pmmg_hip_group`` of include/parmmg_hip.h (device pointers)."""

    _fields_ = [
        ("np", c_int), ("ne", c_int), ("nt", c_int), ("xyz", c_void_p), ("tet8", c_void_p), ("tetv", c_void_p),
        ("adja", c_void_p), ("triv", c_void_p), ("adjt", c_void_p), ("hausd", c_double),
        ("met_size", c_int), ("met", c_void_p), ("nfield", c_int), ("field_size", c_void_p), ("fields", c_void_p),
        ("np_new", c_int), ("xyz_new", c_void_p), ("pclass", c_void_p), ("met_out", c_void_p),
        ("fields_out", c_void_p), ("elem_out", c_void_p), ("hit_out", c_void_p),
    ]


# C-ABI of include/parmmg_hip.h: name -> (restype, argtypes)
HIP_API = {
    "pmmg_hip_abi_version": (c_int, []),
    "pmmg_hip_stats_size": (c_int64, []),
    "pmmg_hip_create": (c_void_p, [c_int, c_int]),
    "pmmg_hip_destroy": (None, [c_void_p]),
    "pmmg_hip_set_background": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p,
                                        c_void_p, c_double, c_int]),
    "pmmg_hip_set_background_tet8": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                             c_double, c_int]),
    "pmmg_hip_set_solutions": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int]),
    "pmmg_hip_locate_interp": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, P(HipStats), c_int]),
    "pmmg_hip_set_point_map": (c_int, [c_void_p, c_int, c_void_p, c_int]),
    "pmmg_hip_start_elements": (c_int, [c_void_p, c_void_p, c_void_p, c_int]),
    "pmmg_hip_sync": (c_int, [c_void_p, P(HipStats)]),
    "pmmg_hip_locate_interp_groups": (c_int, [c_void_p, c_int, c_void_p, P(HipStats)]),
    "pmmg_hip_keep": (c_int, [c_void_p, c_int]),
    "pmmg_hip_carry_over": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "pmmg_hip_bytes_up": (c_int64, [c_void_p, c_int]),
    "pmmg_hip_release_scratch": (c_int, [c_void_p]),
    "pmmg_hip_malloc": (c_void_p, [c_void_p, c_int64]),
    "pmmg_hip_free": (c_int, [c_void_p, c_void_p]),
    "pmmg_hip_build_adjacency": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "pmmg_hip_build_boundary": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                        c_void_p, c_void_p, c_void_p]),
    "pmmg_hip_set_solutions_packed": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int]),
    "pmmg_hip_compute_wgt_mesh": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                          c_void_p, c_int, c_void_p]),
    "pmmg_hip_compute_wgt_faces": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                           c_void_p]),
    "pmmg_hip_tetra_qual": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                    P(c_double)]),
    "pmmg_hip_qual_histo_size": (c_int64, []),
    "pmmg_hip_len_histo_size": (c_int64, []),
    "pmmg_hip_qual_histo": (c_int, [c_void_p, c_int, c_void_p, c_void_p, P(HipQualHisto)]),
    "pmmg_hip_edge_lengths": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                      P(HipLenHisto), c_int, c_void_p, c_void_p]),
    "pmmg_hip_mesh_stats_bytes": (c_int64, [c_void_p]),
    "pmmg_hip_metis_graph": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                     c_int, P(c_int64), c_void_p, c_void_p, c_void_p]),
    "pmmg_hip_part_subgroups": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                        P(c_int), c_int, P(HipSubgroup), P(c_int64), P(c_int)]),
    "pmmg_hip_fix_contiguity": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, P(c_int64),
                                        P(c_int), P(c_int)]),
    "pmmg_hip_contig_passes": (c_int64, [c_void_p]),
    "pmmg_hip_split_groups": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                      c_void_p, c_int, c_int, P(HipSplitCount), c_int64, c_int64, c_int64, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, P(c_int), P(c_int)]),
    "pmmg_hip_gather_rows": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p]),
    "pmmg_hip_split_rounds": (c_int, [c_void_p]),
    "pmmg_hip_merge_groups": (c_int, [c_void_p, c_int, P(HipSplitCount), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_int, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, P(c_int), P(c_int)]),
    "pmmg_hip_gather_rows_i32": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p]),
    "pmmg_hip_ifc_seed": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                  c_void_p]),
    "pmmg_hip_ifc_layers": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, P(c_int), P(c_int),
                                    c_void_p]),
    "pmmg_hip_remap_colors": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                      P(c_int)]),
    "pmmg_hip_memcpy_h2d": (c_int, [c_void_p, c_void_p, c_void_p, c_int64]),
    "pmmg_hip_memcpy_d2h": (c_int, [c_void_p, c_void_p, c_void_p, c_int64]),
    "pmmg_hip_locate_interp_rec": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_int]),
    "pmmg_hip_comm_unique_id": (c_int, [c_void_p]),
    "pmmg_hip_comm_init": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "pmmg_hip_comm_attach": (c_int, [c_void_p, c_void_p, c_int, c_int]),
    "pmmg_hip_allgather_points": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p]),
    "pmmg_hip_last_error": (c_char_p, [c_void_p]),
    "pmmg_hip_device_count": (c_int, []),
}

SYNTH_API = {
    "synth_counts": (c_int, [c_int, c_int, P(c_int64)]),
    "synth_vertices": (c_int, [c_int, c_int, c_double, ctypes.c_uint64, c_void_p, c_void_p]),
    "synth_vertices_valid": (c_int, [c_int, c_int, c_double, ctypes.c_uint64, c_void_p, c_void_p]),
    "synth_tetra": (c_int, [c_int, c_int, c_void_p, c_void_p]),
    "synth_trias": (c_int64, [c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "synth_field": (c_int, [c_int, c_int64, c_void_p, c_void_p]),
    "synth_field_size": (c_int, [c_int]),
    "synth_visit_order": (c_int64, [c_int, c_void_p, c_int, c_void_p]),
    "synth_classes": (c_int, [c_int64, c_void_p, c_int, c_void_p]),
}

_cache: dict[str, ctypes.CDLL] = {}


def _load(path: str, api: dict, what: str) -> ctypes.CDLL:
    if path in _cache:
        return _cache[path]
    if not os.path.exists(path):
        raise RuntimeError(f"{what} is not built ({path}); run `python -m parmmg_amd.build` "
                           "(there is no fallback path)")
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in api.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _cache[path] = lib
    return lib


def hip_lib() -> ctypes.CDLL:
    """The product HIP module (include/parmmg_hip.h)."""
    # PMMG_HIP_SO: an alternative build of the same module (A/B measurements)
    lib = _load(os.environ.get("PMMG_HIP_SO", _build.HIP_SO), HIP_API, "libpmmg_hip.so")
    # the load-time ABI check a shim makes (include/parmmg_hip.h, PMMG_HIP_ABI_VERSION)
    if (lib.pmmg_hip_qual_histo_size() != ctypes.sizeof(HipQualHisto)
            or lib.pmmg_hip_len_histo_size() != ctypes.sizeof(HipLenHisto)):
        raise RuntimeError(f"libpmmg_hip.so report structs {lib.pmmg_hip_qual_histo_size()} / "
                           f"{lib.pmmg_hip_len_histo_size()} B, expected {ctypes.sizeof(HipQualHisto)} / "
                           f"{ctypes.sizeof(HipLenHisto)} B: rebuild (python -m parmmg_amd.build)")
    if lib.pmmg_hip_abi_version() != ABI_VERSION or lib.pmmg_hip_stats_size() != ctypes.sizeof(HipStats):
        raise RuntimeError(f"libpmmg_hip.so ABI {lib.pmmg_hip_abi_version()} / stats {lib.pmmg_hip_stats_size()} B, "
                           f"expected {ABI_VERSION} / {ctypes.sizeof(HipStats)} B: rebuild (python -m parmmg_amd.build)")
    return lib


def synth_lib() -> ctypes.CDLL:
    return _load(_build.SYNTH_SO, SYNTH_API, "libpmmg_synth.so")


HOST_API = {
    "pmmg_classify_points": (c_int64, [c_void_p, c_void_p]),
    "pmmg_copy_metrics_and_fields_point": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int]),
    "pmmg_set_constant_metric": (c_int, [c_void_p]),
    "pmmg_interp_metrics_and_fields": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, P(HipStats)]),
    "pmmg_interp_metrics_and_fields_map": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, P(HipStats)]),
    "pmmg_interp_metrics_and_fields_carry": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                                     P(HipStats)]),
    "pmmg_graph_mesh_elts2metis": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int,
                                           P(P(c_int)), P(P(c_int)), P(P(c_int)), P(c_int64)]),
    "pmmg_host_free": (None, [c_void_p]),
    "pmmg_check_part_contiguity": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "pmmg_fix_contiguity_split": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "pmmg_part_move_interfaces": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                          c_void_p, c_int, c_void_p, P(c_int), P(c_int)]),
    "pmmg_split_grps": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, P(HostSplitResult)]),
    "pmmg_split_result_free": (None, [P(HostSplitResult)]),
    "pmmg_merge_grps": (c_int, [c_void_p, c_int, P(HipSplitCount), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, P(HostMergeResult)]),
    "pmmg_merge_result_free": (None, [P(HostMergeResult)]),
    "pmmg_max_tet_extent": (c_double, [c_int, c_void_p, c_int, c_void_p]),
    "pmmg_shard_mark": (c_int, [c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_double, c_void_p,
                                c_void_p, P(c_int64)]),
    "pmmg_shard_mark_cells": (c_int, [c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_double,
                                      c_void_p, c_void_p, c_double, c_void_p, c_void_p, P(c_int64)]),
    "pmmg_shard_fill": (c_int64, [c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p]),
    "pmmg_shard_mark_trias": (c_int64, [c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "pmmg_shard_fill_region": (c_int64, [c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p]),
    "pmmg_shard_part_pack": (c_int64, [c_void_p, c_void_p, c_void_p, c_int64]),
    "pmmg_shard_assemble": (c_int, [c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pmmg_medit_read_mesh": (c_int, [ctypes.c_char_p, c_void_p, ctypes.c_char_p, c_int]),
    "pmmg_medit_read_sol": (c_int, [ctypes.c_char_p, c_void_p, ctypes.c_char_p, c_int]),
    "pmmg_medit_free_mesh": (None, [c_void_p]),
    "pmmg_medit_free_sol": (None, [c_void_p]),
}


def host_lib() -> ctypes.CDLL:
    hip_lib()  # resolve the dependency from the same directory first
    return _load(_build.HOST_SO, HOST_API, "libpmmg_host.so")
