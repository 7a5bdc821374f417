"""bench.py --dump-outputs (host side): what the timed path computed is written as float32 .npy files, large arrays as the same
seeded sample in every run with their flat indices beside them, 64 MB at most; and --steps is the number of timed steps."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_is_a_fixed_sample_within_the_budget(tmp_path):
    import bench
    g = torch.Generator().manual_seed(0)
    arrays = {"big": torch.rand(3, bench.DUMP_SAMPLES + 12345, generator=g),
              "small": torch.rand(4, 5, generator=g, dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), {k: v.clone() for k, v in arrays.items()})
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["big.npy", "big_index.npy", "small.npy"]
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
    idx = np.load(tmp_path / "a" / "big_index.npy")
    assert idx.dtype == np.float64 and idx.size == bench.DUMP_SAMPLES and np.all(np.diff(idx) > 0)
    big = np.load(tmp_path / "a" / "big.npy")
    assert big.dtype == np.float32 and np.array_equal(big, arrays["big"].numpy().reshape(-1)[idx.astype(np.int64)])
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), arrays["small"].float().numpy().reshape(-1))
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20


def _bench(*args):
    env = dict(os.environ, BENCH_REHEARSAL="dry", HIP_VISIBLE_DEVICES="-1")      # a dry rehearsal uses no device
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, "bench.py", *args], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)


def test_steps_sets_the_timed_steps():
    import json
    r = _bench("--steps", "5", "--warmup", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert line["steps"] == 5 and line["ms_per_step"] > 0
    assert _bench("--steps", "0").returncode != 0


def test_dump_outputs_refused_without_a_device(tmp_path):
    r = _bench("--steps", "2", "--warmup", "0", "--dump-outputs", str(tmp_path / "d"))
    assert r.returncode != 0 and "--dump-outputs" in r.stderr and not os.path.exists(tmp_path / "d")


def test_plain_run_is_the_headline_and_full_adds_the_rest(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3"])
    a = bench.parse()
    assert not a.full and a.no_detail and a.no_extras and a.no_cpu_baseline
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-extras"])
    a = bench.parse()
    assert a.full and not a.no_detail and a.no_extras and not a.no_cpu_baseline
    r = _bench("--steps", "2", "--warmup", "0", "--full")
    assert r.returncode == 0, r.stderr[-2000:]
