"""CPU: bench.py --dump-outputs writes what the last timed step handed its caller (stand-in engine, tests/stub_engine.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from tests.stub_engine import StubEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGV = ["--gpus", "1", "--warmup", "2", "--config", "xlstm_tiny", "--batch", "6"]


def _run(monkeypatch, steps, out_dir):
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LRAM_DIST_SINGLE_RANK"):
        monkeypatch.delenv(k, raising=False)
    engines = []

    def factory(spec, batch, device):
        engines.append(StubEngine(spec, batch, device))
        return engines[-1]

    out = bench.main(ARGV + ["--steps", str(steps), "--dump-outputs", str(out_dir)], engine_factory=factory)
    return out, engines[0]


def _load(d):
    return {n: np.load(os.path.join(str(d), n + ".npy")) for n in ("actions", "tokens")}


def test_dump_holds_the_last_timed_step_and_repeats_exactly(monkeypatch, tmp_path):
    out, eng = _run(monkeypatch, 3, tmp_path / "a")
    assert eng.steps == 2 + 3                                   # W warm-up + exactly K timed steps
    got = _load(tmp_path / "a")
    assert sorted(os.listdir(str(tmp_path / "a"))) == ["actions.npy", "tokens.npy"]
    assert got["actions"].dtype == np.float32 and got["tokens"].dtype == np.float64
    assert np.array_equal(got["actions"], out["last_actions"].numpy())
    assert np.array_equal(got["tokens"], np.round(got["actions"].astype(np.float64) * 64))  # the stand-in's tokens of them
    # the same arguments give the same inputs: a second run writes the same files
    _run(monkeypatch, 3, tmp_path / "b")
    again = _load(tmp_path / "b")
    assert all(np.array_equal(got[n], again[n]) for n in got)
    # --steps moves the last timed step along the seeded episode schedule (returns-to-go fall every step)
    out4, eng4 = _run(monkeypatch, 4, tmp_path / "c")
    assert eng4.steps == 2 + 4 and not np.array_equal(_load(tmp_path / "c")["actions"], got["actions"])


def test_dump_from_two_ranks_holds_the_gathered_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "2", "--config",
           "xlstm_tiny", "--global-batch", "7", "--dump-outputs", str(tmp_path),
           "--engine-factory", os.path.join(ROOT, "tests", "stub_engine.py") + ":factory"]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    got = _load(tmp_path)
    assert got["actions"].shape == got["tokens"].shape == (7, 4)
    assert np.array_equal(got["actions"], np.asarray(line["last_actions"], dtype=np.float32))
    assert np.array_equal(got["tokens"], np.round(got["actions"].astype(np.float64) * 64))


def test_dump_above_the_limit_keeps_one_fixed_row_sample(monkeypatch, tmp_path):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1000)
    g = torch.Generator().manual_seed(5)
    actions = torch.rand(100, 8, generator=g)
    tokens = torch.randint(0, 274, (100, 8), generator=g, dtype=torch.int32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"actions": actions, "tokens": tokens})
    files = sorted(os.listdir(str(tmp_path / "a")))
    assert files == ["actions.npy", "rows.npy", "tokens.npy"]
    arrays = {n: np.load(str(tmp_path / "a" / n)) for n in files}
    assert sum(a.nbytes for a in arrays.values()) <= 1000
    rows = arrays["rows.npy"]
    assert rows.dtype == np.float64 and len(rows) > 0 and np.all(np.diff(rows) > 0)
    idx = rows.astype(np.int64)
    assert np.array_equal(arrays["actions.npy"], actions.numpy()[idx])
    assert np.array_equal(arrays["tokens.npy"], tokens.numpy()[idx].astype(np.float64))
    assert all(np.array_equal(arrays[n], np.load(str(tmp_path / "b" / n))) for n in files)   # the same sample every time


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_refuses_a_step_count_it_cannot_time(argv):
    with pytest.raises(SystemExit):
        bench.parse_args(argv)
