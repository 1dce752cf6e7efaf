"""CPU checks of the invariance helpers of tests/parity.py and of the oracle
they are used with: before a GPU test blames the module for depending on the
frame, the tetra orientation or an array's address, the helper that built the
input — and the reference's own behaviour under it — is pinned here.

  * uniform power-of-two scalings (hausd scaled alike) leave the oracle's
    elem / hit / loc and every output row bit-identical: the reference is
    scale-free on these inputs;
  * shifts keep the hit kinds, and every class (i) point keeps its tetra;
  * flip_orientation gives a valid adjacency over the same geometry, negative
    volumes exactly where it says, and the oracle locates every point in the
    same element;
  * device_view / GuardedAlloc place the payload and notice a touched guard
    byte (over a stand-in for the C-ABI's memory calls in host memory);
  * assert_stats_match accepts the counters of an oracle run restated as
    pmmg_hip_stats and refuses a miscount."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from parity import (EPS, GUARD_BYTE, HIT_COUNTERS, TRANSFORMS, assert_stats_match, check, device_view, flip_case,
                    flip_orientation, make_case, outside_case, same_outputs, step_cap, transform_case, unlocatable)
from parmmg_amd import synth

C, S = synth.CUBE, synth.SHELL
FIXTURES = {"cube-6-7": dict(kind=C, n_old=6, n_new=7), "shell-8-12": dict(kind=S, n_old=8, n_new=12),
            "cube-jitterbg-10-13": dict(kind=C, n_old=10, n_new=13, jitter_old=0.15)}
SHIFTS = {"shift-pow2": (1024.0, -2048.0, 512.0), "shift-1e6": (1e6, 1e6, -1e6), "shift-neg": (-3.25, -3.25, -3.25)}


@pytest.fixture(scope="module")
def cases():
    return {name: make_case(**spec) for name, spec in FIXTURES.items()}


def as_gpu(ref):
    """an oracle run in the module's output form (hit = kind | loc << 4)"""
    loc = np.where(ref["loc"] >= 0, ref["loc"], 0).astype(np.int32)
    return dict(met=ref["met"], fields=ref["fields"], elem=ref["elem"],
                hit=(ref["hit"].astype(np.int32) | (loc << 4)).astype(np.int8))


def volumes(bg):
    p = bg.xyz[bg.tetv - 1]
    return np.einsum("ij,ij->i", p[:, 1] - p[:, 0], np.cross(p[:, 2] - p[:, 0], p[:, 3] - p[:, 0])) / 6.0


@pytest.mark.parametrize("exp", [-20, 20, -60])
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_oracle_is_scale_free(cases, name, exp):
    case = cases[name]
    s = 2.0 ** exp
    t = transform_case(case, s, 0.0, hausd_scale=s)
    assert np.array_equal(t["bg"].xyz, case["bg"].xyz * s) and np.array_equal(t["new"].xyz, case["new"].xyz * s)
    assert t["hausd"] == case["hausd"] * s and t["met"] is case["met"]
    for key in ("ref", "ref_faithful"):
        a, b = case[key], t[key]
        same_outputs(a, b)
        np.testing.assert_array_equal(a["loc"], b["loc"])
    # the transformed case meets its own contract (check() on the oracle's run in the new frame)
    rep = check(t, as_gpu(t["ref"]))
    assert rep["n"] == int((case["pclass"] != 0).sum()) and rep["class_i"] == rep["class_i_same"]


@pytest.mark.parametrize("shift", sorted(SHIFTS))
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_oracle_under_shifts(cases, name, shift):
    case = cases[name]
    t = transform_case(case, 1.0, SHIFTS[shift])
    np.testing.assert_array_equal(t["bg"].xyz, case["bg"].xyz + np.array(SHIFTS[shift]))
    a, b = case["ref"], t["ref"]
    np.testing.assert_array_equal(a["hit"], b["hit"])
    cls_i = np.isin(a["hit"], (1, 2)) & (a["minbary"] > EPS)
    assert cls_i.sum() > 0.5 * (case["pclass"] == 1).sum()
    np.testing.assert_array_equal(a["elem"][cls_i], b["elem"][cls_i])


def test_transform_anisotropic_axes(cases):
    case = cases["cube-6-7"]
    t = transform_case(case, (1.0, 1.0, 2.0 ** -10), (0.0, 0.0, 0.0))
    np.testing.assert_array_equal(t["bg"].xyz[:, :2], case["bg"].xyz[:, :2])
    np.testing.assert_array_equal(t["bg"].xyz[:, 2], case["bg"].xyz[:, 2] * 2.0 ** -10)
    np.testing.assert_array_equal(t["new"].xyz[:, 2], case["new"].xyz[:, 2] * 2.0 ** -10)
    assert t["hausd"] == case["hausd"] and t["bg"].tetv is case["bg"].tetv
    rep = check(t, as_gpu(t["ref"]))
    assert rep["class_i"] == rep["class_i_same"]


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_flip_orientation(cases, name):
    case = cases[name]
    bg = case["bg"]
    fb, flipped = flip_orientation(bg, frac=0.3, seed=3)
    assert 0.2 * bg.ne < flipped.sum() < 0.4 * bg.ne
    assert fb.xyz is bg.xyz and fb.triv is bg.triv
    # the same tetra, every flipped one with the negated volume
    np.testing.assert_array_equal(np.sort(fb.tetv, axis=1), np.sort(bg.tetv, axis=1))
    v0, v1 = volumes(bg), volumes(fb)
    assert (v0 > 0).all() and (v1[flipped] < 0).all() and (v1[~flipped] > 0).all()
    np.testing.assert_allclose(np.abs(v1), v0, rtol=1e-12)
    # a valid adjacency: adja[adja[k, i]] points back at (k, i) and the two faces hold the same vertices
    adja, tetv = fb.adja, fb.tetv
    assert ((adja > 0).sum(axis=1) == (bg.adja > 0).sum(axis=1)).all()
    for k0 in range(fb.ne):
        for i in range(4):
            a = int(adja[k0, i])
            if a == 0:
                continue
            k1, j = (a >> 2) - 1, a & 3
            assert adja[k1, j] == 4 * (k0 + 1) + i, (k0, i, a)
            assert set(np.delete(tetv[k0], i)) == set(np.delete(tetv[k1], j)), (k0, i, a)
    # the reference finds every point in the same element
    f = flip_case(case, frac=0.3, seed=3)
    for key in ("ref", "ref_faithful"):
        np.testing.assert_array_equal(f[key]["elem"], case[key]["elem"])
        np.testing.assert_array_equal(f[key]["hit"], case[key]["hit"])
    in_flipped = f["flipped"][f["ref"]["elem"][case["pclass"] == 1] - 1]
    assert in_flipped.mean() >= 0.2, in_flipped.mean()  # the GPU test's premise
    rep = check(f, as_gpu(f["ref"]))
    assert rep["n"] == int((case["pclass"] != 0).sum()) and rep["class_i"] == rep["class_i_same"]


@pytest.mark.parametrize("transform", [None] + sorted(TRANSFORMS))
def test_closest_start_is_the_references(transform):
    """The reference's closest-tetra search starts from closestDist = 1e10
    (src/locate_pmmg.c:801, :455): an absolute constant.  For the ten points
    of outside_case that no tetra accepts, |min bary| * vol is below it in
    every frame of the invariance tests but the scale 2^20 (~4e16 there): the
    oracle then keeps no tetra (the reference goes on with closestTet = 0),
    and unlocatable() names exactly those points."""
    case = outside_case()
    if transform is not None:
        case = transform_case(case, *TRANSFORMS[transform])
    B, x = case["B"], case["new"].xyz
    out = [i for i in np.nonzero(case["pclass"] == 1)[0] if O.first_accepting_tetra(B, x[i]) == 0]
    assert len(out) == 10
    keys = np.array([min(O.closest_value(B, k, x[i]) for k in range(1, case["bg"].ne + 1)) for i in out[:3]])
    closest = np.array([O.closest_tetra(B, x[i]) for i in out])
    if transform == "scale-2^20":
        assert (keys >= 1e10).all() and (closest == 0).all()
        np.testing.assert_array_equal(unlocatable(case), out)
    else:
        assert (keys < 1e10).all() and (closest > 0).all()
        assert unlocatable(case).size == 0


class _HostMemory:
    """pmmg_hip_malloc / memcpy / free over host memory: what device_view needs of the C-ABI"""

    def __init__(self):
        self.bufs = {}

    def pmmg_hip_malloc(self, h, n):
        raw = ctypes.create_string_buffer(n + 256)
        addr = (ctypes.addressof(raw) + 255) & ~255
        self.bufs[addr] = raw
        return addr

    def pmmg_hip_memcpy_h2d(self, h, dst, src, n):
        ctypes.memmove(dst, src, n)
        return 1

    pmmg_hip_memcpy_d2h = pmmg_hip_memcpy_h2d

    def pmmg_hip_free(self, h, p):
        del self.bufs[p.value]


class _HostCtx:
    h = None

    def __init__(self):
        self.lib = _HostMemory()

    def error(self):
        return "host stand-in"


@pytest.mark.parametrize("offset", [0, 1, 4, 8, 16])
def test_device_view_places_payload_and_guards(offset):
    ctx = _HostCtx()
    a = np.arange(37, dtype=np.float64).reshape(37, 1) if offset % 8 == 0 else np.arange(37, dtype=np.uint8)
    view, alloc = device_view(ctx, a, offset)
    assert view.ptr == alloc.base + 256 + offset and view.ptr % 16 == offset % 16
    assert view.shape == a.shape and view.dtype == a.dtype and view.nbytes == a.nbytes
    np.testing.assert_array_equal(view.download(), a)
    before, after = alloc.zones()
    assert before.size == 256 + offset and after.size == 256
    assert (before == GUARD_BYTE).all() and (after == GUARD_BYTE).all()
    alloc.check()
    # one byte just behind, then one just in front of the payload
    for addr, where in ((view.ptr + a.nbytes, "behind"), (view.ptr - 1, "in front")):
        old = ctypes.c_uint8.from_address(addr).value
        ctypes.c_uint8.from_address(addr).value = 0
        with pytest.raises(AssertionError, match=where):
            alloc.check("x")
        ctypes.c_uint8.from_address(addr).value = old
    alloc.check()
    alloc.free()
    assert view.ptr == 0 and not ctx.lib.bufs


def oracle_stats(case, ref):
    """the counters of an oracle run in pmmg_hip_stats form"""
    pc = case["pclass"]
    kinds = np.bincount(ref["hit"].astype(np.int32) & 15, minlength=16)
    st = {name: int(kinds[h]) for h, name in HIT_COUNTERS.items()}
    steps = np.clip(ref["steps"][pc != 0], 0, 1024)  # (negative: no walk count kept for that point)
    st.update(nvol=int((pc == 1).sum()), nbdy=int((pc == 2).sum()), nvol_exact=0, nvol_src=0, nbdy_src=0,
              nvol_noseed=0, nbdy_fanscan=0, sorted=0, steps_total=int(steps.sum()) + int((pc != 0).sum()),
              stepmax=int(steps.max()), wave_iters=int(steps.sum()) + int((pc != 0).sum()), reserved=[0, 0, 0, 0])
    return st


def test_assert_stats_match_against_oracle_counts(cases):
    case = cases["shell-8-12"]
    ref, pc = case["ref"], case["pclass"]
    st = oracle_stats(case, ref)
    assert_stats_match(st, pc, ref["hit"], sort=False)
    assert_stats_match(st, [pc[:100], pc[100:]], [ref["hit"][:100], ref["hit"][100:]])  # the groups form
    for key, val in (("nvol_walk", st["nvol_walk"] - 1), ("nbdy", st["nbdy"] + 1), ("nbdy_face", st["nbdy_face"] + 1),
                     ("sorted", 1), ("stepmax", step_cap() + 1), ("wave_iters", 0), ("nvol_src", st["nvol"] + 1),
                     ("reserved", [0, 1, 0, 0]), ("steps_total", 3)):
        with pytest.raises(AssertionError):
            assert_stats_match(dict(st, **{key: val}), pc, ref["hit"], sort=False)
    assert step_cap() == 1088 and step_cap(1) == 2 and step_cap(100) == 164
    assert_stats_match(dict(st, stepmax=step_cap(), wave_iters=max(st["wave_iters"], step_cap())), pc, ref["hit"])
    # a hit array that disagrees with the counters
    hit = ref["hit"].copy()
    i = int(np.nonzero(hit == 1)[0][0])
    hit[i] = 2
    with pytest.raises(AssertionError):
        assert_stats_match(st, pc, hit)
    # a volume point left without a hit kind passes only where it is declared
    hit[i] = 0
    lost = dict(st, nvol_walk=st["nvol_walk"] - 1)
    assert_stats_match(lost, pc, hit, unlocated=1)
    for n in (0, 2):
        with pytest.raises(AssertionError):
            assert_stats_match(lost, pc, hit, unlocated=n)
