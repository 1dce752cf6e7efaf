"""Point map, the pieces that need no device: the host layer's
pmmg_interp_metrics_and_fields_map refuses missing arguments without touching
anything, the C-ABI entry points refuse a NULL context, the two counters sit
where the first two reserved words of pmmg_hip_stats were, and the synthetic
maps of parmmg_amd.synth are what they claim to be (CPU only)."""
import ctypes

import numpy as np

from parmmg_amd import _native, synth
from parmmg_amd.transfer import NewGroup, OldGroup


def test_host_function_refuses_null_arguments():
    lib = _native.host_lib()
    olds, news = (OldGroup * 1)(), (NewGroup * 1)()
    st = _native.HipStats()
    st.nvol = 77  # must stay: nothing is touched
    maps = (ctypes.c_void_p * 1)(None)
    po, pn = ctypes.cast(olds, ctypes.c_void_p), ctypes.cast(news, ctypes.c_void_p)
    pm = ctypes.cast(maps, ctypes.c_void_p)
    assert lib.pmmg_interp_metrics_and_fields_map(None, 1, po, pn, 1, pm, ctypes.byref(st)) == 0
    assert lib.pmmg_interp_metrics_and_fields_map(None, 1, None, None, 1, None, None) == 0
    # a context pointer that must never be dereferenced when the group arrays are missing
    bogus = ctypes.c_void_p(8)
    assert lib.pmmg_interp_metrics_and_fields_map(bogus, 1, None, pn, 1, pm, ctypes.byref(st)) == 0
    assert lib.pmmg_interp_metrics_and_fields_map(bogus, 1, po, None, 1, pm, ctypes.byref(st)) == 0
    assert st.nvol == 77


def test_c_abi_refuses_a_null_context():
    lib = _native.hip_lib()
    src = np.ones(4, np.int32)
    out = np.zeros(4, np.int32)
    assert lib.pmmg_hip_set_point_map(None, 4, src.ctypes.data_as(ctypes.c_void_p), 0) == 0
    assert lib.pmmg_hip_start_elements(None, out.ctypes.data_as(ctypes.c_void_p), None, 0) == 0
    assert (out == 0).all()


def test_counters_take_the_first_reserved_words():
    S = _native.HipStats
    assert S.nvol_src.offset == S.nbdy_fanscan.offset + 8
    assert S.nbdy_src.offset == S.nvol_src.offset + 8
    assert S.reserved.offset == S.nbdy_src.offset + 8 and S.reserved.size == 4 * 8
    assert ctypes.sizeof(S) == S.nbdy_fanscan.offset + 8 + 6 * 8  # the size it had with reserved[6]
    assert {"nvol_src", "nbdy_src"} <= set(S().as_dict())


def test_nearest_vertex_map():
    bg = synth.lattice(synth.CUBE, 5)
    new = synth.lattice(synth.CUBE, 6, jitter=0.2, with_tetra=False)
    src = synth.point_map(bg, new.xyz, chunk=37)  # several chunks, the last one short
    assert src.dtype == np.int32 and src.shape == (new.np,)
    d = np.linalg.norm(new.xyz[:, None, :] - bg.xyz[None, :, :], axis=2)
    assert (src >= 1).all() and (src <= bg.np).all()
    np.testing.assert_allclose(d[np.arange(new.np), src - 1], d.min(axis=1), rtol=0, atol=1e-15)


def test_map_from_located_elements():
    bg = synth.lattice(synth.CUBE, 4)
    rng = np.random.default_rng(2)
    n = 200
    pc = rng.integers(0, 3, n).astype(np.uint8)
    elem = np.where(pc == 1, rng.integers(1, bg.ne + 1, n), rng.integers(1, bg.nt + 1, n)).astype(np.int32)
    elem[::17] = 0  # not located
    xyz = rng.uniform(0, 1, (n, 3))
    for stale in (False, True):
        src = synth.point_map(bg, xyz, elem, pc, stale=stale)
        for i in range(n):
            if pc[i] == 0 or elem[i] == 0:
                assert src[i] == 0
                continue
            verts = (bg.tetv if pc[i] == 1 else bg.triv)[elem[i] - 1]
            assert src[i] in verts
            if not stale:
                dist = np.linalg.norm(bg.xyz[verts - 1] - xyz[i], axis=1)
                assert dist[list(verts).index(src[i])] == dist.min()
    a = synth.point_map(bg, xyz, elem, pc, stale=True)
    b = synth.point_map(bg, xyz, elem, pc, stale=True)
    np.testing.assert_array_equal(a, b)  # seeded
