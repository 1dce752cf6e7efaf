"""The closest searches at the edges of their split (pmmg_fallback.hpp,
closest_split), on the smallest background that reaches them.

A closest scan deals the n queries nothing accepted to a grid of G blocks:
groups of 256 queries (or, for a short list, the next power of two with
several lanes per query), nr = G / groups ranges of elements per group, the
ranges' minima in a table the last block merges.  The host picks G from the
background: 64 blocks for the volume and 32 for the surface of the cube
lattice used here (384 tetra, 192 trias).  The lists the other tests present
stay below 401 queries, so these regimes are run here only:

  n = 1, 3          a short list, lanes idle beside the queries' own
  n = 255, 256, 257 the two sides of one full group
  nr == 1           one range per group, the result stored directly and not
                    through the table: from 8193 (volume) / 4097 (surface)
  groups > G        a block takes more than one (group, range) item: from
                    16385 / 8193; with that many fallback queries the query
                    grid of the accept scan is at its cap of 16 cells per axis

The queries are those of tests/test_gpu_fallback_scale.py: volume points
beyond the x = 1 face, surface points 0.05 (5 hausd) off a face, and a few
dozen points inside and on the faces, all under PMMG_HIP_MAXSTEP=1, so the
accept scans and the compaction of the unaccepted queries see both kinds in
one list.  The oracle alone must send every outside / far point down its
closest path (asserted on the CPU, before the device is asked); the device
must then count exactly that many, which shows that the regime was reached.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import oracle as O
from parity import (BDY_CLOSEST, BDY_EXHAUST, BDY_FACE, BDY_STALE, VOL_CLOSEST, VOL_EXHAUST, VOL_WALK,
                    assert_stats_match, make_ctx, run_gpu, same_outputs)
from parmmg_amd import synth
from test_gpu_fallback_scale import HAUSD, _queries

N_OLD = 4  # 6 * 4^3 = 384 tetra, 192 trias: 64 blocks for the volume searches, 32 for the surface ones
N_IN, N_FACE = 40, 40  # points inside and on the faces, beside the outside / far ones
FEW = 3  # the other class's outside / far points while one class is at a size under test
VOL_OUT = (1, 3, 255, 256, 257, 8193, 16385)
BDY_FAR = (1, 3, 255, 257, 4097, 8193)
SEED = 2025


@functools.lru_cache(maxsize=None)
def _background():
    bg = synth.lattice(synth.CUBE, N_OLD)
    assert (bg.ne, bg.nt) == (384, 192)
    met = synth.solution(synth.F_ANI, bg.xyz)
    fields = [synth.solution(synth.F_SCALAR, bg.xyz), synth.solution(synth.F_VECTOR, bg.xyz)]
    return bg, met, fields, O.Background(bg, met, fields, HAUSD)


def edge_case(n_out, n_far):
    """The case (as parity.run_gpu takes it) with n_out volume points outside
    the cube and n_far surface points beyond hausd, and where they are."""
    bg, met, fields, B = _background()
    xyz, pc = _queries(np.random.default_rng(SEED), N_IN, n_out, N_FACE, n_far)
    case = dict(bg=bg, new=SimpleNamespace(xyz=xyz, np=xyz.shape[0]), met=met, fields=fields, pclass=pc, B=B,
                hausd=HAUSD)
    out = np.arange(N_IN, N_IN + n_out)
    far = np.arange(N_IN + n_out + N_FACE, xyz.shape[0])
    return case, out, far


def oracle_codes(case, out, far):
    """What the oracle alone makes of the outside and the far points: each of
    them on its closest path (nothing accepts it, neither on the oracle's
    walk nor in its exhaustive scan).  Returns the oracle's hit codes."""
    xyz, pc, B = case["new"].xyz, case["pclass"], case["B"]
    ref = O.run(B, xyz, pc, np.arange(1, xyz.shape[0] + 1, dtype=np.int32), O.MODE_FRESH)
    code = ref["hit"].astype(np.int32) & 15
    assert (code[out] == VOL_CLOSEST).all(), np.bincount(code[out], minlength=12)
    assert np.isin(code[far], (BDY_STALE, BDY_CLOSEST)).all(), np.bincount(code[far], minlength=12)
    # and the others are inside the domain: something accepts each
    rest = np.setdiff1d(np.arange(xyz.shape[0]), np.concatenate([out, far]))
    assert not np.isin(code[rest], (0, VOL_CLOSEST, BDY_STALE, BDY_CLOSEST)).any()
    return code


def _run_edges(n_out, n_far):
    case, out, far = edge_case(n_out, n_far)
    xyz, pc = case["new"].xyz, case["pclass"]
    want = oracle_codes(case, out, far)
    env = {"PMMG_HIP_MAXSTEP": "1"}
    runs = {}
    for sort in (False, True):
        ctx = make_ctx(sort, env)
        try:
            runs[sort] = [run_gpu(case, ctx=ctx, tet8=True) for _ in range(2)]
        finally:
            ctx.close()
    g = runs[False][0]
    s = g["stats"]
    code = g["hit"].astype(np.int32) & 15
    kinds = np.bincount(code, minlength=12)
    print({k: s[k] for k in ("nvol_walk", "nvol_exhaust", "nvol_closest", "nbdy_exhaust", "nbdy_stale",
                             "nbdy_closest")}, kinds)
    # the regime: exactly the outside / far points took the closest searches
    assert s["nvol_closest"] == n_out and s["nbdy_closest"] + s["nbdy_stale"] == n_far
    assert (code[out] == VOL_CLOSEST).all()
    # the count of each hit code, from the oracle: the closest paths' codes point by point (the stale
    # re-evaluation and the nearest vertex are the oracle's choice, not the walk's), and per class the
    # accepted points, which the one-step walk or the accept scan located
    assert (code[far] == want[far]).all()
    assert kinds[VOL_CLOSEST] == n_out and kinds[BDY_STALE] == int((want == BDY_STALE).sum())
    assert kinds[BDY_CLOSEST] == int((want == BDY_CLOSEST).sum())
    assert kinds[VOL_WALK] + kinds[VOL_EXHAUST] == N_IN and kinds[BDY_FACE:BDY_EXHAUST + 1].sum() == N_FACE
    assert kinds[0] == 0
    assert_stats_match(s, pc, g["hit"], sort=False, maxstep=1)
    assert_stats_match(runs[True][0]["stats"], pc, runs[True][0]["hit"], sort=True, maxstep=1)
    # every point against the oracle
    rep = O.check_batch(case["B"], xyz, pc, g["elem"], g["hit"], g["met"], g["fields"])
    print(rep)
    assert rep["unprocessed"] == 0 and rep["accept_fail"] == 0 and rep["value_fail"] == 0
    assert rep["n"] == xyz.shape[0] and rep["maxrel"] <= 1e-12
    # the same bytes from a second call on the context and in the other query order
    for other in (runs[False][1], runs[True][0], runs[True][1]):
        same_outputs(g, other)


@pytest.mark.gpu
@pytest.mark.parametrize("n_out", VOL_OUT)
def test_closest_tetra_at_the_edges_of_the_split(n_out):
    _run_edges(n_out, FEW)


@pytest.mark.gpu
@pytest.mark.parametrize("n_far", BDY_FAR)
def test_closest_tria_at_the_edges_of_the_split(n_far):
    _run_edges(FEW, n_far)


def test_oracle_alone_takes_the_closest_paths():
    """The inputs of the GPU cases, on the CPU: the oracle sends every outside
    / far point down its closest path and accepts every other."""
    for n_out, n_far in [(n, FEW) for n in VOL_OUT] + [(FEW, n) for n in BDY_FAR]:
        case, out, far = edge_case(n_out, n_far)
        assert (out.size, far.size) == (n_out, n_far)
        oracle_codes(case, out, far)
