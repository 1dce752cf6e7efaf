"""bench.py: the plain run and its options.

CPU: the writer of --dump-outputs (size cap, seeded sample, processed points
only) and the command line.  GPU: two plain runs of the smallest BASELINE
config with the same arguments, their result lines and written outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")

import bench  # noqa: E402  (ROOT is on sys.path: tests/conftest.py)


def _outputs(n, seed=3):
    rng = np.random.default_rng(seed)
    pc = (np.arange(n) % 9 != 0).astype(np.uint8)  # 1 point in 9 skipped
    mo = rng.random((n, 6))
    fo = [rng.random((n, 1)), rng.random((n, 3))]
    elem = rng.integers(1, 1 << 30, n).astype(np.int32)
    hit = np.where(pc != 0, 1, 0).astype(np.int8)
    return pc, mo, fo, elem, hit


def _load(d, suffix=""):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(suffix + ".npy")}


def test_dump_outputs_whole(tmp_path):
    pc, mo, fo, elem, hit = _outputs(1000)
    rep = bench.dump_outputs(str(tmp_path), pc, mo, fo, elem, hit)
    got = _load(tmp_path)
    assert sorted(got) == ["elem", "field0", "field1", "hit", "met", "sample_index"]
    idx = np.nonzero(pc != 0)[0]
    assert not rep["sampled"] and rep["rows"] == idx.size == rep["rows_processed"]
    assert np.array_equal(got["sample_index"], idx)
    assert np.array_equal(got["met"], mo[idx]) and np.array_equal(got["field1"], fo[1][idx])
    assert np.array_equal(got["elem"], elem[idx]) and np.array_equal(got["hit"], hit[idx])
    for name, a in got.items():
        assert a.dtype == (np.float32 if name == "hit" else np.float64), name
    assert rep["bytes"] == sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path))


def test_dump_outputs_sample_is_capped_and_fixed(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 20000)
    pc, mo, fo, elem, hit = _outputs(5000)
    a, b = tmp_path / "a", tmp_path / "b"
    rep = bench.dump_outputs(str(a), pc, mo, fo, elem, hit)
    bench.dump_outputs(str(b), pc, mo, fo, elem, hit)
    ga, gb = _load(a), _load(b)
    assert rep["sampled"] and rep["rows"] == 20000 // (8 * 10 + 20)
    # 7 headers of 128 bytes beside the rows
    assert rep["bytes"] <= 20000 + 7 * 128
    idx = ga["sample_index"].astype(np.int64)
    assert idx.size == rep["rows"] and np.all(np.diff(idx) > 0) and np.all(pc[idx] != 0)
    assert np.array_equal(ga["met"], mo[idx]) and np.array_equal(ga["elem"], elem[idx])
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k


def test_default_cap_is_under_64_mb():
    assert bench.DUMP_CAP_BYTES + 16 * 128 <= 64 * 10**6


def test_steps_must_be_positive():
    p = subprocess.run([sys.executable, BENCH, "--steps", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=120)
    assert p.returncode == 2 and "--steps" in p.stderr


FULL_ONLY = ("cpu_baseline", "parity", "host_mode", "surface_solo", "mmg_like_order", "shuffled_order",
             "shuffled_order_records", "tetra_qual", "snapshot", "groups", "graded")


@pytest.fixture(scope="module")
def plain_runs(tmp_path_factory):
    runs = []
    for tag in ("a", "b"):
        d = tmp_path_factory.mktemp("dump_" + tag)
        p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--config", "cfg2", "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(d)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           timeout=120, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [x for x in p.stdout.splitlines() if x.strip()]
        assert len(lines) == 1, p.stdout
        runs.append((json.loads(lines[0]), d, p.stderr))
    return runs


@pytest.mark.gpu
def test_plain_run_result_line(plain_runs):
    out, _, err = plain_runs[0]
    print(err[-2000:])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["full"] is False
    assert out["unit"] == "Mpts/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["metric"] == bench.METRIC
    assert out["ms_per_step"] > 0
    pts = out["config"]["located_points_per_step"]
    assert abs(out["value"] - pts / (out["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * out["value"] + 1e-3
    for k in FULL_ONLY:
        assert k not in out, k


@pytest.mark.gpu
def test_plain_run_outputs_repeat(plain_runs):
    (out, da, _), (_, db, _) = plain_runs
    ga, gb = _load(da), _load(db)
    assert sorted(ga) == ["elem", "field0", "hit", "met", "sample_index"]
    rows = out["outputs_dumped"]["rows"]
    assert rows == min(out["outputs_dumped"]["rows_processed"], bench.DUMP_CAP_BYTES // (8 * 2 + 20))
    assert sum(os.path.getsize(os.path.join(da, f)) for f in os.listdir(da)) <= 64 * 10**6
    for k, a in ga.items():
        assert a.shape[0] == rows and a.dtype in (np.float32, np.float64), k
        assert np.array_equal(a, gb[k], equal_nan=True), k
    assert np.all(ga["hit"] != 0) and np.all(ga["elem"] >= 1)
    assert np.isfinite(ga["met"]).all() and np.isfinite(ga["field0"]).all()
