"""bench.py's plain run and --dump-outputs: a plain line carries the headline alone (everything else moved behind
--full), --steps sets the timed steps, and the outputs of the last timed step land as float .npy files, the same ones
from run to run, at most 64 MB in all."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("aof_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_exact_floats(bench, tmp_path):
    blocks = np.zeros((3, 5), dtype=[("dx", "i1"), ("dy", "i1"), ("sad", "<u2")])
    blocks["dx"], blocks["sad"] = -4, 65535
    count = np.array([0, 1, 2 ** 32 - 1], dtype=np.uint32)
    bench.dump_outputs(str(tmp_path), {"blocks": blocks, "count": count, "status": 7})
    got = load_dir(tmp_path)
    assert sorted(got) == ["blocks_dx", "blocks_dy", "blocks_sad", "count", "status"]
    assert got["blocks_dx"].dtype == np.float32 and got["blocks_sad"].dtype == np.float32 and got["blocks_dx"].shape == (3, 5)
    assert (got["blocks_dx"] == -4).all() and (got["blocks_sad"] == 65535).all()
    assert got["count"].dtype == np.float64 and got["count"].tolist() == [0, 1, 2 ** 32 - 1]
    assert got["status"].shape == () and got["status"] == 7


def test_dump_samples_the_same_rows_of_a_large_output(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 40_000)
    rows = np.arange(1000 * 50, dtype=np.uint8).reshape(1000, 50)
    recs = np.arange(1000, dtype=np.int32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"rows": rows, "recs": recs})
    a, b = load_dir(tmp_path / "a"), load_dir(tmp_path / "b")
    assert sorted(a) == ["recs", "recs_index", "rows", "rows_index"]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 40_000 + 4 * 128
    idx = a["rows_index"].astype(np.int64)
    assert 0 < len(idx) < 1000 and np.array_equal(a["rows"], rows[idx].astype(np.float32))
    assert np.array_equal(a["recs"], recs[a["recs_index"].astype(np.int64)].astype(np.float64))


def run_bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                         timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_line_and_its_outputs(tmp_path):
    common = ["--pairs", "16", "--steps", "3", "--warmup", "1", "--settle-steps", "2"]
    j = run_bench(*common, "--dump-outputs", str(tmp_path / "a"))
    assert j["steps"] == 3 and j["ms_per_step"] > 0 and j["value"] > 0 and j["unit"] == "frame-pairs/s"
    assert j["higher_is_better"] and j["dtype"] == "u8" and j["metric"].startswith("frame-pairs/s")
    for key in ("parity", "cpu_baseline", "workloads", "realistic_input", "exhaustive_search", "exact_pruned_search"):
        assert key not in j, key
    assert j["kernels_ms"] is None and j["ms_per_step_median"] is None
    run_bench(*common, "--dump-outputs", str(tmp_path / "b"))
    a, b = load_dir(tmp_path / "a"), load_dir(tmp_path / "b")
    assert {"blocks_dx", "blocks_dy", "blocks_sad", "flows_flow_x", "flows_flow_y", "flows_quality"} <= set(a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert a["flows_flow_x"].shape == (16,) and a["blocks_sad"].shape[0] == 16
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    # baseline input: pure integer translations, every pair's flow is its shift (as the --full line checks)
    assert (np.abs(a["flows_flow_x"]) <= 4).all() and (a["flows_flow_x"] == np.round(a["flows_flow_x"])).all()
    k = run_bench(*common, "--full", "--cpu-seconds", "0", "--traffic", "file", "--legs", "none")
    assert k["steps"] == 3 and k["parity"]["oracle_pairs_bit_exact"] and k["parity"]["all_pairs_return_known_shift"]
    assert k["kernels_ms"]["search"] > 0
