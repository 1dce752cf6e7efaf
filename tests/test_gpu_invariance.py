"""The transfer's result is a function of the query and the background only
(runs on the MI355X): not of the frame the coordinates come in, of the
orientation the tetra are stored with, of the address an array starts at, or
of the number of queries relative to a wave, a scan chunk or a sort tile.

Every other GPU test feeds the module unit-sized meshes around the origin,
positively oriented tetra and arrays on allocation bases.  The helpers of
tests/parity.py (checked on the CPU in test_invariance_host.py) build the
other inputs; every comparison is bit-exact or check()'s contract.

Branches first executed here (from the code; confirmed by the counters the
tests assert):
  * test_frames / test_frames_fallbacks: k_bbox, quant / Frame::qs, the seed,
    surface, binning and fallback query grids and elem_box's padding at
    extents 2^-20 .. 2^20 and at coordinates up to 1e6 times the extent
    (nvol_exhaust + nvol_closest > 0 and the surface fallbacks > 0 under
    PMMG_HIP_MAXSTEP=1);
  * test_orientation: the vol < 0 branch of the fp32 filter (step_f32) and of
    exact_accept with the default walks (at least 20 % of the volume points end
    in an inverted tetra, accepted there by exact_accept), and the exhaustive
    accept scan (k_exhaust_accept<4>: tet_bary and elem_box on inverted
    tetra) under PMMG_HIP_MAXSTEP=1 (nvol_exhaust > 0, inverted tetra among
    its results);
  * test_device_offsets: the scalar side of k_quantize (xyz at +8), of
    cls_bits (pclass at +1; input order, sorted == 0, whose surface list is
    the class compaction) and of k_vol's query-row load (xyz_new at +8; both
    orders run, the input order takes it: the Morton order reads the
    module's own aligned processing-order copy); store6's else-branch with
    the record layout (1, 1, 3, 6) of cube-iso-oddtensor-6-7, the one
    compiled layout whose tensor sits on an odd double (a size-6 row array
    is kept on 16 bytes by the header: test_misaligned_bases_are_refused);
  * test_sizes_at_edges: partial last waves, scan chunks and sort tiles."""
import numpy as np
import pytest

from parity import (EPS, ELEM_SENTINEL, HIT_SENTINEL, ROW_SENTINEL, TRANSFORMS, assert_skipped_keep,
                    assert_stats_match, check, device_view, flip_case, make_case, outside_case, run_dev_views, run_gpu,
                    same_outputs, transform_case, unlocatable)
from parmmg_amd import synth
from parmmg_amd.transfer import TransferContext, pack_solutions, pack_tet8
from test_gpu_parity import MODES, _packed_variant

C, S = synth.CUBE, synth.SHELL
FIXTURES = {"cube-6-7": dict(kind=C, n_old=6, n_new=7), "shell-8-12": dict(kind=S, n_old=8, n_new=12),
            "cube-jitterbg-10-13": dict(kind=C, n_old=10, n_new=13, jitter_old=0.15)}
FRAME_MODES = ["auto", "morton", "tet8", "packed"]
EXACT = ("scale-2^-20", "scale-2^20")  # every device quantity scales exactly: bit-identical to the unscaled run
MAXSTEP1 = {"PMMG_HIP_MAXSTEP": "1"}


class Cache:
    """cases and runs shared by the tests of this module (never modified)"""

    def __init__(self):
        self.cases, self.runs = {}, {}

    def case(self, name, transform=None, flip=False):
        key = (name, transform, flip)
        if key not in self.cases:
            if transform is not None:
                self.cases[key] = transform_case(self.case(name), *TRANSFORMS[transform])
            elif flip:
                self.cases[key] = flip_case(self.case(name), frac=0.3, seed=3)
            else:
                self.cases[key] = make_case(**FIXTURES[name])
        return self.cases[key]

    def base_run(self, name, mode):
        """the untransformed, unflipped GPU run"""
        if (name, mode) not in self.runs:
            case = self.case(name)
            if MODES[mode].get("packed"):
                case = _packed_variant(case)
            self.runs[name, mode] = run_gpu(case, **MODES[mode])
        return self.runs[name, mode]


@pytest.fixture(scope="module")
def cache():
    return Cache()


def full_check(case, gpu, **stats_kw):
    rep = check(case, gpu)
    assert rep["n"] == int((case["pclass"] != 0).sum())
    assert rep["class_i"] == rep["class_i_same"]  # (check() raises on the first class (i) point that moved)
    assert_stats_match(gpu["stats"], case["pclass"], gpu["hit"], **stats_kw)
    return rep


def with_env(mode, env):
    kw = dict(MODES[mode])
    kw["env"] = {**kw.get("env", {}), **env}
    return kw


# ---------------------------------------------------------------- 2. frames

@pytest.mark.gpu
@pytest.mark.parametrize("transform", sorted(TRANSFORMS))
@pytest.mark.parametrize("mode", FRAME_MODES)
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_frames(cache, name, mode, transform):
    """The parity contract in a scaled, shifted or stretched frame, against the
    oracle of the transformed case, with no point excluded; under the two
    power-of-two scalings the outputs are bit-identical to the unscaled GPU
    run (the oracle is, test_invariance_host.py: a difference is an absolute
    constant in the device code)."""
    case = cache.case(name, transform)
    if MODES[mode].get("packed"):
        case = _packed_variant(case)
    gpu = run_gpu(case, **MODES[mode])
    rep = full_check(case, gpu, sort=MODES[mode].get("sort"))
    print(name, mode, transform, rep, gpu["stats"])
    if transform in EXACT:
        same_outputs(gpu, cache.base_run(name, mode))


@pytest.mark.gpu
@pytest.mark.parametrize("transform", [None] + sorted(TRANSFORMS))
def test_frames_fallbacks(transform):
    """PMMG_HIP_MAXSTEP=1 sends nearly every query of the cube 5 -> 6 (ten
    volume points outside the domain, ten surface points off the surface)
    through the exhaustive and closest kernels: their box padding and query
    grids in every frame.

    One absolute constant is the reference's own: its closest-tetra search
    starts from 1e10 (src/locate_pmmg.c:801), and at scale 2^20 the ten outside
    points' |min bary| * vol is ~4e16, so the reference keeps no tetra for them
    (test_invariance_host.py::test_closest_start_is_the_references).  The module
    must leave exactly those points unprocessed and their rows untouched;
    everything else is checked as in every other frame."""
    case = outside_case()
    if transform is not None:
        case = transform_case(case, *TRANSFORMS[transform])
    lost = unlocatable(case)
    assert lost.size == (10 if transform == "scale-2^20" else 0)
    gpu = run_gpu(case, env=MAXSTEP1)
    np.testing.assert_array_equal(np.nonzero((case["pclass"] != 0) & ((gpu["hit"] & 15) == 0))[0], lost)
    kept = case["pclass"].copy()
    kept[lost] = 0  # check(): rows untouched, no hit kind
    rep = check(dict(case, pclass=kept), gpu)
    assert_skipped_keep(dict(case, pclass=kept), gpu)
    st = gpu["stats"]
    print(transform, rep, st)
    assert rep["n"] == int((kept != 0).sum())
    assert_stats_match(st, case["pclass"], gpu["hit"], maxstep=1, unlocated=lost.size)
    assert st["nvol_exhaust"] + st["nvol_closest"] > 0
    assert st["nbdy_exhaust"] + st["nbdy_closest"] + st["nbdy_stale"] > 0


# ---------------------------------------------------------------- 3. orientation

@pytest.mark.gpu
@pytest.mark.parametrize("maxstep", [None, 1])
@pytest.mark.parametrize("mode", FRAME_MODES)
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_orientation(cache, name, mode, maxstep):
    """30 % of the tetra stored with local vertices 0 and 1 swapped (negative
    volume, adjacency renumbered with them): the vol < 0 branches of the fp32
    filter and of exact_accept (default walks), and the exhaustive accept
    scan over inverted tetra (PMMG_HIP_MAXSTEP=1).  Contract against the flipped background's
    oracle; every class (i) point in the tetra the unflipped GPU run found."""
    case = cache.case(name, flip=True)
    if MODES[mode].get("packed"):
        case = _packed_variant(case)
    gpu = run_gpu(case, **(with_env(mode, MAXSTEP1) if maxstep else MODES[mode]))
    rep = full_check(case, gpu, sort=MODES[mode].get("sort"), **(dict(maxstep=1) if maxstep else {}))
    print(name, mode, maxstep, rep, gpu["stats"])
    ref, pc = case["ref"], case["pclass"]
    cls_i = (pc == 1) & np.isin(ref["hit"], (1, 2)) & (ref["minbary"] > EPS)
    assert cls_i.sum() == rep["class_i"] > 0
    np.testing.assert_array_equal(gpu["elem"][cls_i], cache.base_run(name, mode)["elem"][cls_i])
    in_flipped = case["flipped"][gpu["elem"][pc == 1] - 1]
    assert in_flipped.mean() >= 0.2, in_flipped.mean()
    if maxstep:
        assert gpu["stats"]["nvol_exhaust"] > 0
        assert case["flipped"][gpu["elem"][(gpu["hit"] & 15) == 2] - 1].any()  # an inverted tetra accepted by the scan


# ---------------------------------------------------------------- 4. pointer offsets

PACKABLE = (synth.F_SCALAR, synth.F_VECTOR, synth.F_TENSOR)  # with the aniso metric: sizes 6, 1, 3, 6
OFFSET_CASES = {"cube-jitterbg-10-13": dict(kind=C, n_old=10, n_new=13, jitter_old=0.15, fields=PACKABLE,
                                            req_every=9),  # 2197 points: no multiple of 64
                "shell-8-12": dict(kind=S, n_old=8, n_new=12, fields=PACKABLE, req_every=9),
                # sizes 1, 1, 3, 6: the one compiled record layout with a tensor on an odd double (bytes 40-87
                # of a 96-byte record), whose rows of surface, continued and fallback points go through
                # store6's else-branch
                "cube-iso-oddtensor-6-7": dict(kind=C, n_old=6, n_new=7, metric=synth.F_ISO, fields=PACKABLE,
                                               req_every=9)}
# (separate tetv / adja arrays, packed records in and out, armed point map)
OFFSET_CONFIGS = {"arrays": (True, False, False), "tet8": (False, False, False), "rec": (False, True, False),
                  "map": (False, False, True)}


@pytest.fixture(scope="module")
def offset_cases():
    out = {}
    for name, spec in OFFSET_CASES.items():
        case = make_case(**spec)
        assert (case["pclass"] == 0).any() and (case["pclass"] == 2).any()
        case["src"] = synth.point_map(case["bg"], case["new"].xyz)
        case["checked"] = False
        out[name] = case
    return out


# both forced orders for each layout; one armed call per case (the input order, which streams the map)
OFFSET_RUNS = [(s, c) for c in ("arrays", "tet8", "rec") for s in (False, True)] + [(False, "map")]


@pytest.mark.gpu
@pytest.mark.parametrize("sort,config", OFFSET_RUNS, ids=[("morton-" if s else "input-") + c for s, c in OFFSET_RUNS])
@pytest.mark.parametrize("name", sorted(OFFSET_CASES))
def test_device_offsets(offset_cases, name, sort, config):
    """Device mode with every array at the smallest offset the header allows
    (parity.VIEW_OFFSETS: xyz and xyz_new at +8, pclass and hit_out at +1,
    elem_out, triv, adjt and the map at +4, tetra arrays, size-6 rows and
    records at +16): bit-identical to the same call on aligned arrays (which
    is check()ed once per case), every guard zone around every array intact,
    skipped rows still at their sentinel.  The scalar sides of k_quantize,
    cls_bits (input order) and k_vol's query-row load (input order) run here
    and nowhere else."""
    case = offset_cases[name]
    separate, rec, mapped = OFFSET_CONFIGS[config]
    src = case["src"] if mapped else None
    base = run_dev_views(case, sort, separate=separate, rec=rec, shifted=False, src=src)
    assert_stats_match(base["stats"], case["pclass"], base["hit"], sort=sort)
    if not case["checked"]:
        rep = check(case, base)
        assert rep["n"] == int((case["pclass"] != 0).sum()) and rep["class_i"] == rep["class_i_same"]
        case["checked"] = True
    got = run_dev_views(case, sort, separate=separate, rec=rec, shifted=True, src=src)
    same_outputs(got, base)
    for out in (base, got):
        assert_skipped_keep(case, out, row=ROW_SENTINEL)
    assert_stats_match(got["stats"], case["pclass"], got["hit"], sort=sort)
    for key in ("nvol_src", "nbdy_src", "nvol_exact", "steps_total", "stepmax"):
        assert got["stats"][key] == base["stats"][key], key
    if mapped:
        assert got["stats"]["nvol_src"] > 0 and got["stats"]["nbdy_src"] > 0
    skip = case["pclass"] == 0
    print(name, sort, config, got["stats"], "skipped elem kept:", bool((got["elem"][skip] == ELEM_SENTINEL).all()),
          "skipped hit kept:", bool((got["hit"][skip] == HIT_SENTINEL).all()))


@pytest.mark.gpu
def test_misaligned_bases_are_refused(offset_cases):
    """A base the header forbids — a size-6 row array, packed records, a tetra
    array at +8 — is refused with a message, and nothing runs: the outputs
    and every guard zone keep their fill."""
    case = offset_cases["shell-8-12"]
    bg, new, met, fields, pc = case["bg"], case["new"], case["met"], case["fields"], case["pclass"]
    nq = new.np
    allocs = []

    def dv(ctx, a, off):
        v, al = device_view(ctx, a, off)
        allocs.append(al)
        return v

    with TransferContext(0, sort=False) as ctx:
        xyz, triv, adjt = dv(ctx, bg.xyz, 8), dv(ctx, bg.triv, 4), dv(ctx, bg.adjt, 4)
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            ctx.set_background(xyz, dv(ctx, bg.tetv, 8), dv(ctx, bg.adja, 16), triv, adjt, case["hausd"])
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            ctx.set_background(xyz, dv(ctx, bg.tetv, 16), dv(ctx, bg.adja, 8), triv, adjt, case["hausd"])
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            ctx.set_background_tet8(xyz, dv(ctx, pack_tet8(bg.tetv, bg.adja), 8), triv, adjt, case["hausd"])
        ctx.set_background_tet8(xyz, dv(ctx, pack_tet8(bg.tetv, bg.adja), 16), triv, adjt, case["hausd"])
        with pytest.raises(RuntimeError, match="16-byte aligned"):  # a tensor metric at +8
            ctx.set_solutions(dv(ctx, met, 8), [dv(ctx, f, 16 if f.shape[1] == 6 else 8) for f in fields])
        with pytest.raises(RuntimeError, match="16-byte aligned"):  # a tensor field at +8
            ctx.set_solutions(dv(ctx, met, 16), [dv(ctx, f, 8) for f in fields])
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            ctx.set_solutions_packed(dv(ctx, pack_solutions(met, fields), 8), 6, [f.shape[1] for f in fields])
        ctx.set_solutions(dv(ctx, met, 16), [dv(ctx, f, 16 if f.shape[1] == 6 else 8) for f in fields])
        q, pcd = dv(ctx, new.xyz, 8), dv(ctx, pc, 1)
        el, hit = dv(ctx, np.full(nq, ELEM_SENTINEL, np.int32), 4), dv(ctx, np.full(nq, HIT_SENTINEL, np.int8), 1)
        sizes = [met.shape[1]] + [f.shape[1] for f in fields]
        outs = [dv(ctx, np.full((nq, s), ROW_SENTINEL), 8) for s in sizes]  # the size-6 outputs at +8
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            ctx.locate_interp(q, pcd, outs[0], outs[1:], el, hit)
        ctx.sync()
        ctx.set_solutions_packed(dv(ctx, pack_solutions(met, fields), 16), 6, [f.shape[1] for f in fields])
        ro = dv(ctx, np.full((nq, 16), ROW_SENTINEL), 8)
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            ctx.locate_interp_rec(q, pcd, ro, el, hit)
        ctx.sync()
        want = np.array([ROW_SENTINEL]).view(np.uint64)[0]
        for o in outs + [ro]:
            assert (o.download().view(np.uint64) == want).all()
        assert (el.download() == ELEM_SENTINEL).all() and (hit.download() == HIT_SENTINEL).all()
        for al in allocs:
            al.check()
            al.free()


def host_view(a, fill=None):
    """(view, buffer): a C-contiguous view that starts one element into a larger buffer"""
    a = np.ascontiguousarray(a)
    buf = np.full(a.size + 2, 0 if fill is None else fill, a.dtype)
    v = buf[1:1 + a.size].reshape(a.shape)
    if fill is None:
        v[...] = a
    return v, buf


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["nosort", "morton", "tet8"])
@pytest.mark.parametrize("name", sorted(OFFSET_CASES))
def test_host_views_one_element_in(offset_cases, name, mode):
    """Host mode through numpy views that start one element into a larger
    buffer (what a shim passes: met->m + met->size, mesh->adja + 1): identical
    to the plain call, the elements around every output untouched."""
    case = offset_cases[name]
    bg, new = case["bg"], case["new"]
    plain = run_gpu(case, **MODES[mode])
    V = lambda a: host_view(a)[0]  # noqa: E731
    nq = new.np
    with TransferContext(0, sort=MODES[mode].get("sort")) as ctx:
        if MODES[mode].get("tet8"):
            ctx.set_background_tet8(V(bg.xyz), V(pack_tet8(bg.tetv, bg.adja)), V(bg.triv), V(bg.adjt), case["hausd"])
        else:
            ctx.set_background(V(bg.xyz), V(bg.tetv), V(bg.adja), V(bg.triv), V(bg.adjt), case["hausd"])
        ctx.set_solutions(V(case["met"]), [V(f) for f in case["fields"]])
        sizes = [case["met"].shape[1]] + [f.shape[1] for f in case["fields"]]
        outs = [host_view(np.empty((nq, s)), fill=np.nan) for s in sizes]
        el, hit = host_view(np.empty(nq, np.int32), fill=0), host_view(np.empty(nq, np.int8), fill=0)
        for _, buf in outs + [el, hit]:
            buf[0], buf[-1] = 99, 99
        st = ctx.locate_interp(V(new.xyz), V(case["pclass"]), outs[0][0], [o[0] for o in outs[1:]], el[0], hit[0])
    got = dict(met=outs[0][0], fields=[o[0] for o in outs[1:]], elem=el[0], hit=hit[0])
    same_outputs(got, plain)
    for _, buf in outs + [el, hit]:
        assert buf[0] == 99 and buf[-1] == 99
    assert_stats_match(st, case["pclass"], got["hit"], sort=MODES[mode].get("sort"))
    assert_skipped_keep(case, got)


# ---------------------------------------------------------------- 5. sizes at wave, scan-chunk and sort-tile edges

EDGE_SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193]  # 64: a wave; 4096: kScanChunk and kRsTile


@pytest.fixture(scope="module")
def edge_pool():
    """the cube 8 -> 20 with its 9261 new points shuffled once"""
    case = make_case(kind=C, n_old=8, n_new=20, fields=PACKABLE, with_ref=False)
    perm = np.random.default_rng(20).permutation(case["new"].np)
    case["perm"], case["pc_all"] = perm, synth.classes(case["new"])
    return case


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_sizes_at_edges(edge_pool, n):
    """The first n shuffled points (classes as generated, every 7th skipped)
    in forced input order and forced Morton order, array and packed solutions:
    the contract on up to 1500 points, every other point processed, and the
    two orders bit-identical (the walk is a function of the query alone)."""
    import dataclasses
    pool = edge_pool
    ids = pool["perm"][:n]
    pc = pool["pc_all"][ids].copy()
    pc[6::7] = 0
    new = dataclasses.replace(pool["new"], xyz=np.ascontiguousarray(pool["new"].xyz[ids]),
                              isbdy=np.ascontiguousarray(pool["new"].isbdy[ids]))
    case = dict(pool, new=new, pclass=pc)
    for packed in (False, True):
        kw = dict(tet8=True, packed=True) if packed else {}
        a = run_gpu(case, sort=False, **kw)
        b = run_gpu(case, sort=True, **kw)
        same_outputs(a, b)
        rep = check(case, a, max_points=1500)
        assert rep["n"] == min(1500, int((pc != 0).sum()))
        assert ((a["hit"] & 15) != 0).sum() == (pc != 0).sum()
        assert_stats_match(a["stats"], pc, a["hit"], sort=False)
        assert_stats_match(b["stats"], pc, b["hit"], sort=True)
        assert_skipped_keep(case, a)
        assert_skipped_keep(case, b)
