"""bench.py's launcher contract, on CPU (no GPU is touched).

`python bench.py --gpus N` without a launcher must start N ranks itself (torch.distributed.run
as a child process) and must refuse, with a non-zero exit, to measure fewer ranks than asked.
"""
import json
import os
import subprocess
import sys

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def _env():
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    return env


def test_launcher_spawns_n_ranks_dry_run():
    for n in (2, 4, 8):
        out = subprocess.run([sys.executable, BENCH, "--gpus", str(n), "--steps", "20", "--warmup", "5",
                              "--dry-run-launch"], capture_output=True, text=True, env=_env(), timeout=120)
        assert out.returncode == 0, out.stderr
        d = json.loads(out.stdout.strip().splitlines()[-1])
        cmd = d["launch"]
        assert cmd[1:3] == ["-m", "torch.distributed.run"]
        assert cmd[cmd.index("--nproc-per-node") + 1] == str(n)
        assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
        assert os.path.samefile(cmd[cmd.index("--master-port") + 2], BENCH)
        # the ranks get the same flags, so their world-size check sees --gpus N
        assert cmd[cmd.index("--gpus") + 1] == str(n) and "--dry-run-launch" not in cmd
        assert d["nproc"] == n


def test_launcher_refuses_without_enough_gpus():
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "2"], capture_output=True,
                         text=True, env=_env(), timeout=120)
    assert out.returncode == 2
    assert "refusing" in out.stderr


def test_dump_outputs_writes_float64_npy(tmp_path, monkeypatch):
    """--dump-outputs: x, f_hist, f_hist_best and fval as float64 .npy; an x beyond the per-array
    cap is stored as the same seeded sample of its entries in every run."""
    import numpy as np
    import torch

    import bench
    x = torch.arange(24, dtype=torch.float32).reshape(6, 4)
    res = {"f_hist": [np.float64(3.0), np.float64(2.0)], "f_hist_best": [np.float64(3.0), np.float64(2.0)],
           "fval": np.float64(2.0)}
    shapes = bench.dump_outputs(str(tmp_path / "a"), x, res)
    assert shapes == {"x": [6, 4], "f_hist": [2], "f_hist_best": [2], "fval": [1]}
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in shapes}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["x"], x.numpy()) and np.array_equal(got["f_hist"], [3.0, 2.0])
    assert got["fval"][0] == 2.0
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8 * 10)
    bench.dump_outputs(str(tmp_path / "b"), x, res)
    bench.dump_outputs(str(tmp_path / "c"), x, res)
    xb, xc = np.load(tmp_path / "b" / "x.npy"), np.load(tmp_path / "c" / "x.npy")
    assert xb.shape == (10,) and np.array_equal(xb, xc)
    assert np.all(np.diff(xb) > 0) and set(xb) <= set(range(24))


def test_rank_world_mismatch_is_an_error():
    env = _env()
    env.update(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, BENCH, "--gpus", "8", "--steps", "2"], capture_output=True,
                         text=True, env=env, timeout=120)
    assert out.returncode == 2
    assert "WORLD_SIZE=1" in out.stderr
