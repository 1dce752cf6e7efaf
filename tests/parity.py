"""Parity checking of the HIP module against the CPU oracle.

Contract (BASELINE.json north_star):
  (i)   a volume point whose reference tetra has min barycentric coordinate
        > MMG5_EPS is located in the IDENTICAL tetra (surface face hits are
        only reported: near domain edges a tria of the adjacent face can accept
        the point within hausd, so the reference's own answer is path dependent);
  (ii)  every other point lands in an element the reference accepts (walk /
        wedge / cone criteria), or in the reference's exhaustive result
        (lowest-index accepting element, else the closest element);
  (iii) the interpolated metric and fields equal the reference interpolator
        evaluated in the element the module chose — checked bit for bit
        (tolerance written here: 1e-12 relative, and the exact-match count is
        reported).
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from parmmg_amd import synth
from parmmg_amd.transfer import TransferContext

EPS = O.EPS
REL_TOL = 1e-12

VOL_WALK, VOL_EXHAUST, VOL_CLOSEST = 1, 2, 3
BDY_FACE, BDY_EDGE, BDY_VERTEX, BDY_WEDGE, BDY_CONE, BDY_EXHAUST, BDY_STALE, BDY_CLOSEST = range(4, 12)


def make_case(kind=synth.CUBE, n_old=6, n_new=7, metric=synth.F_ANI,
              fields=(synth.F_SCALAR, synth.F_VECTOR, synth.F_TENSOR, synth.F_AFFINE),
              jitter_old=0.0, jitter_new=0.2, req_every=0, hausd=0.01, seed=synth.SEED, with_ref=True):
    bg = synth.lattice(kind, n_old, jitter=jitter_old)
    new = synth.lattice(kind, n_new, jitter=jitter_new, seed=seed)
    met = None if metric is None else synth.solution(metric, bg.xyz)
    fs = [synth.solution(w, bg.xyz) for w in fields]
    pc = synth.classes(new, req_every)
    B = O.Background(bg, met, fs, hausd)
    case = dict(bg=bg, new=new, met=met, fields=fs, pclass=pc, B=B, hausd=hausd)
    if with_ref:
        vis = synth.visit_order(new)
        case["ref"] = O.run(B, new.xyz, pc, vis, O.MODE_FRESH)
        case["ref_faithful"] = O.run(B, new.xyz, pc, vis, O.MODE_FAITHFUL)
    return case


def make_ctx(sort=None, env=None):
    """A context created under the PMMG_HIP_* settings of env (read by
    pmmg_hip_create only; the environment is restored)."""
    import os
    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        return TransferContext(0, sort=sort)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_gpu(case, sort=None, ctx=None, tet8=False, packed=False, env=None):
    """env: PMMG_HIP_* settings read when the context is created (documented
    options and test-only path selection, e.g. PMMG_HIP_BINBITS=7: the fine
    Morton cells auto mode picks for a numbering without coherence)."""
    bg, new = case["bg"], case["new"]
    own = ctx is None
    ctx = ctx or make_ctx(sort, env)
    try:
        if tet8:
            from parmmg_amd.transfer import pack_tet8
            ctx.set_background_tet8(bg.xyz, pack_tet8(bg.tetv, bg.adja), bg.triv, bg.adjt, case["hausd"])
        else:
            ctx.set_background(bg.xyz, bg.tetv, bg.adja, bg.triv, bg.adjt, case["hausd"])
        if packed:
            from parmmg_amd.transfer import pack_solutions
            ctx.set_solutions_packed(pack_solutions(case["met"], case["fields"]),
                                     0 if case["met"] is None else case["met"].shape[1],
                                     [f.shape[1] for f in case["fields"]])
        else:
            ctx.set_solutions(case["met"], case["fields"])
        npn = new.np
        met_out = None if case["met"] is None else np.full((npn, case["met"].shape[1]), np.nan)
        f_out = [np.full((npn, f.shape[1]), np.nan) for f in case["fields"]]
        elem = np.zeros(npn, np.int32)
        hit = np.zeros(npn, np.int8)
        st = ctx.locate_interp(new.xyz, case["pclass"], met_out, f_out, elem, hit)
        return dict(met=met_out, fields=f_out, elem=elem, hit=hit,
                    stats=dict(st.as_dict(), reserved=list(st.reserved)))
    finally:
        if own:
            ctx.close()


def run_dev(ctx, bg, new_xyz, met, fields, pc, hausd, separate=False, packed=False):
    """One transfer with every array resident on the device (the bench's
    device mode): returns (met, fields, elem, hit) downloaded + the stats."""
    from parmmg_amd.transfer import pack_tet8

    nq = new_xyz.shape[0]
    d = dict(xyz=ctx.upload(bg.xyz), triv=ctx.upload(bg.triv), adjt=ctx.upload(bg.adjt), q=ctx.upload(new_xyz),
             pc=ctx.upload(pc))
    if separate:
        d["tetv"], d["adja"] = ctx.upload(bg.tetv), ctx.upload(bg.adja)
        ctx.set_background(d["xyz"], d["tetv"], d["adja"], d["triv"], d["adjt"], hausd)
    else:
        d["tet8"] = ctx.upload(pack_tet8(bg.tetv, bg.adja))
        ctx.set_background_tet8(d["xyz"], d["tet8"], d["triv"], d["adjt"], hausd)
    if packed:
        from parmmg_amd.transfer import pack_solutions
        d["rec"] = ctx.upload(pack_solutions(met, fields))
        ctx.set_solutions_packed(d["rec"], 0 if met is None else met.shape[1], [f.shape[1] for f in fields])
    else:
        d["met"] = None if met is None else ctx.upload(met)
        d["f"] = [ctx.upload(f) for f in fields]
        ctx.set_solutions(d["met"], d["f"])
    mo = None if met is None else ctx.empty((nq, met.shape[1]), np.float64)
    fo = [ctx.empty((nq, f.shape[1]), np.float64) for f in fields]
    el, hit = ctx.empty((nq,), np.int32), ctx.empty((nq,), np.int8)
    ctx.locate_interp(d["q"], d["pc"], mo, fo, el, hit, sync=False)
    st = ctx.sync()
    out = (None if mo is None else mo.download(), [f.download() for f in fo], el.download(), hit.download(), st)
    for a in [x for x in d.values() if x is not None] + [mo, el, hit] + fo:
        for b in (a if isinstance(a, list) else [a]):
            if b is not None:
                b.free()
    return out


# ---------------------------------------------------------------- invariance helpers
#
# The transfer's result is a function of the query and the background only:
# not of the frame the coordinates are given in, of the orientation the tetra
# are stored with, of where the arrays start in memory, or of what the context
# did before.  The helpers below build the inputs that say so.

def transform_case(case, scale3=1.0, shift3=0.0, hausd_scale=1.0):
    """The case under x -> scale * x + shift (per axis), applied to the
    background's and the new points' coordinates; the solutions keep their
    values (fields of the vertices, not of the frame).  hausd is multiplied by
    hausd_scale.  B, ref and ref_faithful are rebuilt in the new frame.  A
    power-of-two scale with a zero shift is exact in binary."""
    import dataclasses
    s = np.broadcast_to(np.asarray(scale3, np.float64), (3,))
    t = np.broadcast_to(np.asarray(shift3, np.float64), (3,))

    def mv(m):
        x = m.xyz * s
        if np.any(t != 0.0):
            x = x + t
        return dataclasses.replace(m, xyz=np.ascontiguousarray(x), extra=dict(m.extra))

    bg, new = mv(case["bg"]), mv(case["new"])
    hausd = case["hausd"] * hausd_scale
    out = dict(case, bg=bg, new=new, hausd=hausd, B=O.Background(bg, case["met"], case["fields"], hausd))
    out.pop("ref", None)
    out.pop("ref_faithful", None)
    if "ref" in case:
        vis = synth.visit_order(new)
        out["ref"] = O.run(out["B"], new.xyz, case["pclass"], vis, O.MODE_FRESH)
        out["ref_faithful"] = O.run(out["B"], new.xyz, case["pclass"], vis, O.MODE_FAITHFUL)
    return out


# the frames of the invariance tests: name -> (scale per axis, shift per axis, hausd factor)
TRANSFORMS = {
    "scale-2^-20": (2.0 ** -20, 0.0, 2.0 ** -20),
    "scale-2^20": (2.0 ** 20, 0.0, 2.0 ** 20),
    "shift-pow2": (1.0, (1024.0, -2048.0, 512.0), 1.0),
    "shift-1e6": (1.0, (1e6, 1e6, -1e6), 1.0),
    "shift-neg": (1.0, (-3.25, -3.25, -3.25), 1.0),
    "slab-z-2^-10": ((1.0, 1.0, 2.0 ** -10), 0.0, 1.0),  # thinner than hausd
    "stretch-x-2^10": ((2.0 ** 10, 1.0, 1.0), 0.0, 1.0),
}


def flip_orientation(bg, frac=0.3, seed=0):
    """(mesh, flipped): the same geometry with local vertices 0 and 1 of a
    random share `frac` of the tetra swapped — their adja entries 0 and 1 with
    them, and face index 0 <-> 1 in every 4k+i code that points at such a
    tetra.  Every flipped tetra has the negated (negative) volume; flipped is
    the boolean mask per tetra."""
    import dataclasses
    rng = np.random.default_rng(seed)
    flipped = rng.random(bg.ne) < frac
    tetv, adja = bg.tetv.copy(), bg.adja.copy()
    tetv[flipped, 0], tetv[flipped, 1] = bg.tetv[flipped, 1], bg.tetv[flipped, 0]
    adja[flipped, 0], adja[flipped, 1] = bg.adja[flipped, 1], bg.adja[flipped, 0]
    k, i = adja >> 2, adja & 3
    swap = (adja > 0) & flipped[np.maximum(k, 1) - 1] & (i < 2)
    adja = np.where(swap, 4 * k + (i ^ 1), adja).astype(np.int32)
    mesh = dataclasses.replace(bg, tetv=np.ascontiguousarray(tetv), adja=np.ascontiguousarray(adja),
                               extra=dict(bg.extra))
    return mesh, flipped


def flip_case(case, frac=0.3, seed=0):
    """The case over flip_orientation's background (same queries, solutions and
    hausd; B, ref and ref_faithful rebuilt); case["flipped"] is the mask."""
    bg, flipped = flip_orientation(case["bg"], frac, seed)
    out = dict(case, bg=bg, flipped=flipped, B=O.Background(bg, case["met"], case["fields"], case["hausd"]))
    if "ref" in case:
        vis = synth.visit_order(case["new"])
        out["ref"] = O.run(out["B"], case["new"].xyz, case["pclass"], vis, O.MODE_FRESH)
        out["ref_faithful"] = O.run(out["B"], case["new"].xyz, case["pclass"], vis, O.MODE_FAITHFUL)
    return out


GUARD_BYTE = 0xA5


class GuardedAlloc:
    """One device allocation [guard | offset | payload | guard] made by
    device_view; every byte outside the payload was set to GUARD_BYTE."""

    def __init__(self, ctx, base, guard, offset, nbytes, view):
        self.ctx, self.base, self.guard, self.offset, self.nbytes, self.view = ctx, base, guard, offset, nbytes, view

    def zones(self):
        """(before, after): the bytes in front of and behind the payload, downloaded"""
        import ctypes
        total = 2 * self.guard + self.offset + self.nbytes
        buf = np.empty(total, np.uint8)
        if not self.ctx.lib.pmmg_hip_memcpy_d2h(self.ctx.h, buf.ctypes.data_as(ctypes.c_void_p),
                                                ctypes.c_void_p(self.base), total):
            raise RuntimeError(self.ctx.error())
        lo = self.guard + self.offset
        return buf[:lo], buf[lo + self.nbytes:]

    def check(self, what=""):
        before, after = self.zones()
        bad_b, bad_a = np.nonzero(before != GUARD_BYTE)[0], np.nonzero(after != GUARD_BYTE)[0]
        assert bad_b.size == 0, f"{what}: {bad_b.size} bytes written in front of the array, nearest at " \
                                f"-{before.size - int(bad_b[-1])}"
        assert bad_a.size == 0, f"{what}: {bad_a.size} bytes written behind the array, first at +{int(bad_a[0])}"

    def free(self):
        import ctypes
        if self.base:
            self.ctx.lib.pmmg_hip_free(self.ctx.h, ctypes.c_void_p(self.base))
            self.base = 0
            self.view.ptr = 0


def device_view(ctx, array, offset_bytes, guard=256):
    """(view, alloc): `array` uploaded offset_bytes past a guard zone inside a
    larger allocation that is filled with GUARD_BYTE first.  view is a
    DeviceArray on that (deliberately offset) address which does not own the
    memory — release it with alloc.free(), never view.free(); alloc.check()
    downloads both zones around the payload and asserts they are untouched."""
    import ctypes
    from parmmg_amd.transfer import DeviceArray
    a = np.ascontiguousarray(array)
    total = 2 * guard + offset_bytes + a.nbytes
    base = ctx.lib.pmmg_hip_malloc(ctx.h, total)
    if not base:
        raise RuntimeError(ctx.error())
    assert base % 256 == 0 and guard % 256 == 0, "the offset is meant to be the array's whole misalignment"
    fill = np.full(total, GUARD_BYTE, np.uint8)
    ok = ctx.lib.pmmg_hip_memcpy_h2d(ctx.h, ctypes.c_void_p(base), fill.ctypes.data_as(ctypes.c_void_p), total)
    ptr = base + guard + offset_bytes
    if ok and a.nbytes:
        ok = ctx.lib.pmmg_hip_memcpy_h2d(ctx.h, ctypes.c_void_p(ptr), a.ctypes.data_as(ctypes.c_void_p), a.nbytes)
    if not ok:
        raise RuntimeError(ctx.error())
    view = DeviceArray(ptr, a.nbytes, a.shape, a.dtype, ctx)
    return view, GuardedAlloc(ctx, base, guard, offset_bytes, a.nbytes, view)


def outside_case(n_out=10, **kw):
    """The cube 5 -> 6 with n_out volume points pushed outside the background
    (the walks get stuck: exhaustive scan, then the closest tetra), five
    surface points beyond hausd under the bottom face (exhaustive -> stale /
    closest) and five within hausd of it; no oracle run (with_ref=False)."""
    case = make_case(**{**dict(kind=synth.CUBE, n_old=5, n_new=6, with_ref=False), **kw})
    new = case["new"]
    rng = np.random.default_rng(7)
    vol = np.nonzero(case["pclass"] == 1)[0]
    bdy = np.nonzero(case["pclass"] == 2)[0]
    pick_v = rng.choice(vol, n_out, replace=False)
    pick_b = rng.choice(bdy, 10, replace=False)
    new.xyz[pick_v, 0] = 1.0 + rng.uniform(0.001, 0.2, n_out)
    new.xyz[pick_b[:5], 2] = -0.05
    new.xyz[pick_b[5:], 2] = -0.004
    case["B"] = O.Background(case["bg"], case["met"], case["fields"], case["hausd"])
    return case


# byte offsets of the device arrays of run_dev_views: the smallest the header
# allows per array (tetra arrays, size-6 rows and packed records need 16 bytes)
VIEW_OFFSETS = dict(xyz=8, q=8, s1=8, s3=8, tetv=16, adja=16, tet8=16, s6=16, rec=16, triv=4, adjt=4, elem=4, src=4,
                    pclass=1, hit=1)
ROW_SENTINEL = np.array([0x7FF8DEAD0000BEEF], np.uint64).view(np.float64)[0]  # a NaN with a payload of its own
ELEM_SENTINEL, HIT_SENTINEL = -77, 0x40  # (hit: kind 0 in bits 0-3)


def run_dev_views(case, sort, separate=False, rec=False, shifted=True, src=None, env=None):
    """run_dev's transfer on a fresh context with every array behind
    device_view: at VIEW_OFFSETS past a 256-byte-aligned address (shifted) or
    on it.  Outputs are pre-filled with the sentinels.  After the call every
    guard zone of every array, inputs included, is checked.  rec: packed
    records in, pmmg_hip_locate_interp_rec out.  src: a point map, armed from
    device memory.  Returns the outputs and stats like run_gpu."""
    from parmmg_amd.transfer import pack_solutions, pack_tet8
    bg, new, met, fields, pc = case["bg"], case["new"], case["met"], case["fields"], case["pclass"]
    ctx = make_ctx(sort, env)
    allocs = {}

    def dv(name, arr, kind):
        view, allocs[name] = device_view(ctx, arr, VIEW_OFFSETS[kind] if shifted else 0)
        return view

    def rows(name, a):
        return dv(name, a, "s%d" % a.shape[1])

    try:
        nq = new.np
        xyz, triv, adjt = dv("xyz", bg.xyz, "xyz"), dv("triv", bg.triv, "triv"), dv("adjt", bg.adjt, "adjt")
        if separate:
            ctx.set_background(xyz, dv("tetv", bg.tetv, "tetv"), dv("adja", bg.adja, "adja"), triv, adjt,
                               case["hausd"])
        else:
            ctx.set_background_tet8(xyz, dv("tet8", pack_tet8(bg.tetv, bg.adja), "tet8"), triv, adjt, case["hausd"])
        sizes = ([] if met is None else [met.shape[1]]) + [f.shape[1] for f in fields]
        if rec:
            ctx.set_solutions_packed(dv("rec", pack_solutions(met, fields), "rec"),
                                     0 if met is None else met.shape[1], [f.shape[1] for f in fields])
        else:
            ctx.set_solutions(None if met is None else rows("met", met),
                              [rows("f%d" % j, f) for j, f in enumerate(fields)])
        q, pcd = dv("q", new.xyz, "q"), dv("pclass", pc, "pclass")
        el = dv("elem", np.full(nq, ELEM_SENTINEL, np.int32), "elem")
        hit = dv("hit", np.full(nq, HIT_SENTINEL, np.int8), "hit")
        if src is not None:
            ctx.set_point_map(dv("src", np.ascontiguousarray(src, np.int32), "src"))
        if rec:
            rs = (sum(sizes) + 1) & ~1
            ro = dv("rec_out", np.full((nq, rs), ROW_SENTINEL), "rec")
            ctx.locate_interp_rec(q, pcd, ro, el, hit, sync=False)
        else:
            outs = [rows("out%d" % j, np.full((nq, s), ROW_SENTINEL)) for j, s in enumerate(sizes)]
            ctx.locate_interp(q, pcd, outs[0] if met is not None else None, outs[1:] if met is not None else outs,
                              el, hit, sync=False)
        st = ctx.sync()
        if rec:
            r, got, o = ro.download(), [], 0
            for s in sizes:
                got.append(np.ascontiguousarray(r[:, o:o + s]))
                o += s
            pad = r[:, o:]
            assert np.array_equal(pad.view(np.uint64), np.full(pad.shape, ROW_SENTINEL).view(np.uint64)) or \
                not pad.size, "the records' padding was written"
        else:
            got = [o.download() for o in outs]
        out = dict(met=got[0] if met is not None else None, fields=got[1:] if met is not None else got,
                   elem=el.download(), hit=hit.download(), stats=dict(st.as_dict(), reserved=list(st.reserved)))
        for name, al in allocs.items():
            al.check(name)
        return out
    finally:
        for al in allocs.values():
            al.free()
        ctx.close()


def assert_skipped_keep(case, out, row=np.nan, elem=None, hit=None):
    """the rows of skipped points still hold what they were pre-filled with"""
    skip = case["pclass"] == 0
    want = np.array([row], np.float64).view(np.uint64)[0]
    for a in ([out["met"]] if out["met"] is not None else []) + out["fields"]:
        assert (np.ascontiguousarray(a[skip]).view(np.uint64) == want).all(), "a skipped point's row was written"
    if elem is not None:
        assert (out["elem"][skip] == elem).all(), "a skipped point's elem_out was written"
    if hit is not None:
        assert (out["hit"][skip] == hit).all(), "a skipped point's hit_out was written"


HIT_COUNTERS = {VOL_WALK: "nvol_walk", VOL_EXHAUST: "nvol_exhaust", VOL_CLOSEST: "nvol_closest",
                BDY_FACE: "nbdy_face", BDY_EDGE: "nbdy_edge", BDY_VERTEX: "nbdy_vertex", BDY_WEDGE: "nbdy_wedge",
                BDY_CONE: "nbdy_cone", BDY_EXHAUST: "nbdy_exhaust", BDY_STALE: "nbdy_stale",
                BDY_CLOSEST: "nbdy_closest"}
DEFAULT_MAXSTEP = 1024  # the walks' step cap without PMMG_HIP_MAXSTEP
FILTER_STEPS = 64       # the fp32 filter walk's own cap (pmmg_hip_ctx::filter_steps)


def step_cap(maxstep=DEFAULT_MAXSTEP):
    """The most steps one query can count under PMMG_HIP_MAXSTEP = maxstep: a
    volume query walks at most min(FILTER_STEPS, maxstep) steps in the fp32
    filter, and the exact walk that continues from there has the cap maxstep
    of its own (k_vol adds the two counts; a surface walk has the one cap)."""
    return maxstep + min(maxstep, FILTER_STEPS)


def unlocatable(case):
    """The volume points the reference itself cannot place: no tetra accepts
    them and none has |min bary| * vol below the 1e10 its closest search
    starts from (src/locate_pmmg.c:801; closestTet stays 0, and the reference
    goes on with tetra[0]).  An absolute constant the module shares: it
    leaves such a point unprocessed.  Indices, by the oracle's scans."""
    B, x = case["B"], case["new"].xyz
    return np.array([i for i in np.nonzero(case["pclass"] == 1)[0]
                     if O.first_accepting_tetra(B, x[i]) == 0 and O.closest_tetra(B, x[i]) == 0], np.int64)


def assert_stats_match(stats, pclass, hit, sort=None, maxstep=DEFAULT_MAXSTEP, unlocated=0):
    """pmmg_hip_stats against the pclass / hit_out arrays it summarises
    (arrays or lists of arrays: the groups call sums over its groups).  stats: a
    HipStats or its dict; sort: the order forced at pmmg_hip_create (None:
    either); maxstep: PMMG_HIP_MAXSTEP in force (see step_cap); unlocated: the
    number of volume points the reference cannot place either (unlocatable),
    counted in nvol and in no hit kind."""
    if not isinstance(stats, dict):
        stats = dict(stats.as_dict(), reserved=list(stats.reserved))
    def cat(a):
        return np.concatenate([np.ravel(x) for x in a]) if isinstance(a, (list, tuple)) else np.asarray(a)

    pc, code = cat(pclass), cat(hit).astype(np.int32) & 15
    nvol, nbdy = int((pc == 1).sum()), int((pc == 2).sum())
    assert (stats["nvol"], stats["nbdy"]) == (nvol, nbdy), (stats, nvol, nbdy)
    kinds = np.bincount(code, minlength=16)
    for h, name in HIT_COUNTERS.items():
        assert stats[name] == int(kinds[h]), (name, stats[name], int(kinds[h]))
    assert stats["nvol_walk"] + stats["nvol_exhaust"] + stats["nvol_closest"] == nvol - unlocated
    assert sum(stats[HIT_COUNTERS[h]] for h in range(BDY_FACE, BDY_CLOSEST + 1)) == nbdy
    # the kinds belong to the classes they are counted for
    assert int((code[pc == 1] == 0).sum()) == unlocated
    assert np.isin(code[pc == 1], (0, VOL_WALK, VOL_EXHAUST, VOL_CLOSEST)).all()
    assert ((code[pc == 2] >= BDY_FACE) & (code[pc == 2] <= BDY_CLOSEST)).all()
    assert (code[pc == 0] == 0).all()
    ngroups = len(pclass) if isinstance(pclass, (list, tuple)) else 1  # (a groups call counts its binned groups)
    if sort is not None:
        assert stats["sorted"] == ngroups * int(bool(sort)), stats["sorted"]
    assert 0 <= stats["sorted"] <= ngroups, stats["sorted"]
    assert 0 <= stats["stepmax"] <= step_cap(maxstep), (stats["stepmax"], maxstep)
    walk_hits = int(kinds[VOL_WALK]) + int(kinds[BDY_FACE:BDY_CONE + 1].sum())
    assert stats["steps_total"] >= walk_hits, (stats["steps_total"], walk_hits)
    assert stats["wave_iters"] >= stats["stepmax"], (stats["wave_iters"], stats["stepmax"])
    assert 64 * stats["wave_iters"] >= stats["steps_total"], (stats["wave_iters"], stats["steps_total"])
    for name in ("nvol_exact", "nvol_src", "nvol_noseed"):
        assert 0 <= stats[name] <= nvol, (name, stats[name], nvol)
    for name in ("nbdy_src", "nbdy_fanscan"):
        assert 0 <= stats[name] <= nbdy, (name, stats[name], nbdy)
    if "reserved" in stats:
        assert not any(stats["reserved"]), stats["reserved"]


def same_outputs(a, b):
    """elem, hit and every row of two runs bit-identical (NaN payloads included)"""
    np.testing.assert_array_equal(a["elem"], b["elem"])
    np.testing.assert_array_equal(a["hit"], b["hit"])
    assert (a["met"] is None) == (b["met"] is None) and len(a["fields"]) == len(b["fields"])
    for x, y in zip(([a["met"]] if a["met"] is not None else []) + a["fields"],
                    ([b["met"]] if b["met"] is not None else []) + b["fields"]):
        np.testing.assert_array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64))


def invmat_failure_case():
    """A 4-cell cube whose tensors make MMG5_invmat return 0 on every path
    the reference has for it (rows then left untouched):
      * vertex tensors u u^T (u = (1, 2, 3): off-diagonals >= MMG5_EPS, det
        exactly 0) at the interior vertex (3,3,3) and the boundary vertex
        (0,2,2): the inversion of a vertex tensor fails — interp4bar_ani
        (src/interpmesh_pmmg.c:258-259) for volume points in its tetra,
        interp3bar_ani (:177-178) for surface face hits, interp2bar (:98-99)
        for surface edge hits;
      * the edge (1,1,1)-(2,1,1) and the boundary edge (1,3,0)-(2,3,0) carry
        the tensors 0.5 J - I and I (J = all ones; both invert exactly in
        binary), and a new point sits on each edge's midpoint, where the
        coordinates are exactly (1/2, 1/2, 0, ...): every vertex inverts, but
        mint = 1/2 (J - I) + 1/2 I = 1/2 J is singular and the final inversion
        fails (:107 edge, :187 face, :267 volume).
    The same tensors go into the metric and into the tensor field."""
    case = make_case(kind=synth.CUBE, n_old=4, n_new=5, metric=synth.F_ANI,
                     fields=(synth.F_SCALAR, synth.F_VECTOR, synth.F_TENSOR),
                     with_ref=False)
    bg, new = case["bg"], case["new"]

    def vid(i, j, k):  # the cube lattice's vertex numbering (n = 4: 5 per row)
        v = 1 + i + 5 * j + 25 * k
        assert np.allclose(bg.xyz[v - 1], np.array([i, j, k]) / 4.0)
        return v

    J = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0])  # m11 m12 m13 m22 m23 m33
    I3 = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0])
    rank1 = np.array([1.0, 2.0, 3.0, 4.0, 6.0, 9.0])  # (1,2,3)(1,2,3)^T
    special = {vid(3, 3, 3): rank1, vid(0, 2, 2): rank1,
               vid(1, 1, 1): 0.5 * J - I3, vid(2, 1, 1): I3,
               vid(1, 3, 0): 0.5 * J - I3, vid(2, 3, 0): I3}
    for v, t in special.items():
        case["met"][v - 1] = t
        case["fields"][2][v - 1] = t
    # one volume point and one surface point moved onto the two edge midpoints
    pc = case["pclass"]
    vol = int(np.nonzero(pc == 1)[0][0])
    srf = int(np.nonzero((pc == 2) & (new.xyz[:, 2] == 0.0))[0][0])
    new.xyz[vol] = (0.375, 0.25, 0.25)
    new.xyz[srf] = (0.375, 0.75, 0.0)
    case["B"] = O.Background(bg, case["met"], case["fields"], case["hausd"])
    return case, vol, srf


def _same(a, b):
    """bit-equal or both NaN (rows left untouched by a failed tensor inversion)"""
    return np.all((a == b) | (np.isnan(a) & np.isnan(b)))


def _relerr(a, b):
    d = np.abs(a - b)
    s = np.maximum(np.abs(a), np.abs(b))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(s > 0, d / s, d)
    r = np.where(np.isnan(a) & np.isnan(b), 0.0, r)
    return float(np.nanmax(np.where(np.isnan(r), np.inf, r))) if r.size else 0.0


def check(case, gpu, max_points=None):
    """Return a report dict; raises AssertionError on a contract violation."""
    B, new, pc, ref = case["B"], case["new"], case["pclass"], case.get("ref")
    code = (gpu["hit"].astype(np.int32) & 15)
    loc = (gpu["hit"].astype(np.int32) >> 4) & 3
    rep = dict(n=0, exact=0, maxrel=0.0, class_i=0, class_i_same=0, hits={}, ref_hits={})
    # skipped rows untouched
    skip = pc == 0
    if case["met"] is not None:
        assert np.isnan(gpu["met"][skip]).all(), "skipped rows were written"
    assert (code[skip] == 0).all()
    assert (code[~skip] != 0).all(), f"{int((code[~skip] == 0).sum())} points not processed"
    idx = np.nonzero(~skip)[0]
    if max_points is not None and idx.size > max_points:
        idx = np.random.default_rng(0).choice(idx, max_points, replace=False)
    for c in np.unique(code[idx]):
        rep["hits"][int(c)] = int((code[idx] == c).sum())
    if ref is not None:
        for c in np.unique(ref["hit"][idx]):
            rep["ref_hits"][int(c)] = int((ref["hit"][idx] == c).sum())
    for i in idx:
        x = new.xyz[i]
        is_bdy = pc[i] == 2
        h, k, l = int(code[i]), int(gpu["elem"][i]), int(loc[i])
        # (ii) acceptance of the chosen element
        if h == VOL_WALK:
            assert not is_bdy and O.tetra_minbary(B, k, x) > -EPS, (i, h, k)
        elif h == VOL_EXHAUST:
            assert not is_bdy and k == O.first_accepting_tetra(B, x), (i, h, k)
        elif h == VOL_CLOSEST:
            kb = O.closest_tetra(B, x)
            assert O.first_accepting_tetra(B, x) == 0, (i, h, k)
            # lowest index among exact ties (the reference: first evaluated)
            assert k == kb or O.closest_value(B, k, x) == O.closest_value(B, kb, x), (i, h, k, kb)
        elif h in (BDY_FACE, BDY_EDGE, BDY_VERTEX):
            ok, _ = O.tria_accepts(B, k, x)
            assert is_bdy and ok, (i, h, k)
        elif h == BDY_WEDGE:
            assert O.wedge_test(B, k, l, x) == 4, (i, h, k, l)
        elif h == BDY_CONE:
            assert O.cone_test(B, k, l, x) == 1, (i, h, k, l)
        elif h == BDY_EXHAUST:
            assert k == O.first_accepting_tria(B, x), (i, h, k)
        elif h in (BDY_STALE, BDY_CLOSEST):
            assert O.first_accepting_tria(B, x) == 0 and k == O.closest_tria(B, x), (i, h, k)
        else:
            raise AssertionError(f"unknown hit {h} at {i}")
        # (iii) values = reference arithmetic in the chosen element
        met, fr = O.eval_in_element(B, x, is_bdy, k, h, l)
        got = ([gpu["met"][i]] if met is not None else []) + [f[i] for f in gpu["fields"]]
        want = ([met] if met is not None else []) + fr
        same = all(_same(g, w) for g, w in zip(got, want))
        rel = max(_relerr(g, w) for g, w in zip(got, want))
        rep["exact"] += int(same)
        rep["maxrel"] = max(rep["maxrel"], rel)
        assert rel <= REL_TOL, (i, h, k, rel, got, want)
        rep["n"] += 1
        # (i) identical element where the reference is unambiguous
        if ref is not None:
            rh = int(ref["hit"][i])
            if rh in (VOL_WALK, VOL_EXHAUST) and ref["minbary"][i] > EPS:
                rep["class_i"] += 1
                same_elem = int(ref["elem"][i]) == k
                rep["class_i_same"] += int(same_elem)
                assert same_elem, f"class (i) point {i}: reference elem {ref['elem'][i]} hit {rh}, module elem {k} hit {h}"
            elif rh == BDY_FACE and ref["minbary"][i] > EPS:
                # surface hits are path dependent near domain edges (a tria of
                # the adjacent face may accept within hausd): reported, class (ii)
                rep.setdefault("srf_face", 0)
                rep.setdefault("srf_face_same", 0)
                rep["srf_face"] += 1
                rep["srf_face_same"] += int(int(ref["elem"][i]) == k)
    return rep


def stale_case(hausd: float = 0.01):
    """A surface fixture that reaches the reference's stale re-evaluation
    (src/locate_pmmg.c:505-509): two boundary trias
    without adjacency, T1 = tria 1 horizontal at z = -0.1 (normal +z), T2 =
    tria 2 = the last tria (nt) tilted (normal (-1,-1,2)/sqrt 6), and surface
    points above T2's foot print at |z| < hausd.  Every point is rejected by
    both trias' own tests (T1: 0.1 below, T2: ~0.24 off its plane), the walk
    has no neighbour to step to, so the exhaustive search accepts nothing and
    the closest tria by centroid is T1; the reference then re-evaluates with
    `ptr` still at T2 (the loop's last tria) but T1's normal and index — T2's
    vertices projected along +z enclose the points, so the re-evaluation
    accepts, and the values are T1's vertex values weighted by T2's
    coordinates.  Returns (case, expected) with expected the values of that
    arithmetic restated in numpy (barycoord_pmmg.c:191-223,
    interpmesh_pmmg.c:125-149), independent of the oracle."""
    from parmmg_amd.synth import Mesh

    xyz = np.array([[5, 0, 0], [6, 0, 0.5], [5, 1, 0.5], [5.1, 0.1, -0.1], [5.6, 0.1, -0.1], [5.1, 0.6, -0.1],
                    [5.1, 0.1, -0.6]], np.float64)
    tetv = np.array([[4, 5, 7, 6]], np.int32)  # one positive tetra under T1 (the volume is not queried)
    triv = np.array([[4, 5, 6], [1, 2, 3]], np.int32)
    bg = Mesh(synth.CUBE, 0, xyz, tetv, np.zeros((1, 4), np.int32), triv, np.zeros((2, 3), np.int32), None)
    q = np.array([[5.3, 0.3, 0.005], [5.2, 0.5, -0.004], [5.25, 0.2, 0.0]], np.float64)
    new = Mesh(synth.CUBE, 0, q, np.zeros((0, 4), np.int32), np.zeros((0, 4), np.int32), np.zeros((0, 3), np.int32),
               np.zeros((0, 3), np.int32), None)
    met = np.arange(1, 8, dtype=np.float64)[:, None]
    fs = [np.stack([np.arange(7) * 10.0 + 1, np.arange(7) ** 2 + 0.5, -np.arange(7) * 3.0], 1)]
    pc = np.full(q.shape[0], 2, np.uint8)  # PMMG_PT_BDY
    case = dict(bg=bg, new=new, met=met, fields=fs, pclass=pc, B=O.Background(bg, met, fs, hausd), hausd=hausd)
    # the stale arithmetic: T2's vertices, T1's unit normal, T2's area (|non-unit normal|, locate_pmmg.c:82)
    p1, p2 = xyz[triv[0] - 1], xyz[triv[1] - 1]
    n1 = np.cross(p1[1] - p1[0], p1[2] - p1[0])
    n1 /= np.linalg.norm(n1)
    q2 = np.linalg.norm(np.cross(p2[1] - p2[0], p2[2] - p2[0]))
    exp_met, exp_f = [], []
    for x in q:
        dist = np.dot(x - p2[0], n1)
        proj = x - dist * n1
        phi = [np.dot(np.cross(p2[(i + 1) % 3] - proj, p2[(i + 2) % 3] - proj), n1) / q2 for i in range(3)]
        exp_met.append(sum(phi[i] * met[triv[0][i] - 1] for i in range(3)))
        exp_f.append(sum(phi[i] * fs[0][triv[0][i] - 1] for i in range(3)))
    return case, dict(met=np.array(exp_met), fields=[np.array(exp_f)], elem=1)
