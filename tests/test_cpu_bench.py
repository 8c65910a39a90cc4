"""CPU tests of bench.py's contract plumbing: `python bench.py --gpus N` starts N ranks itself (the driver's
scaling runs call it that way) and the process group it builds has exactly N ranks; the algorithmic work per
utterance reproduces SURVEY §8(d)'s flop-counter figures for the configs BASELINE.json names."""
import json
import os
import subprocess
import sys

from conftest import ROOT


def test_bench_gpus_flag_spawns_that_many_ranks():
    env = dict(os.environ, FDDM_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run"], env=env,
                         capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    rec = json.loads(line)
    assert rec["n_gpus"] == 2 and rec["parallelism"] == "dp2" and rec["global_batch"] == 64


def test_bench_rejects_world_size_mismatch():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run"], env=env,
                         capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode != 0 and "--gpus is 2" in out.stderr


def test_plain_run_is_the_default_and_full_is_opt_in():
    import bench
    sys.argv = ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"]
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    sys.argv = ["bench.py", "--full", "--dump-outputs", "somewhere"]
    a = bench.parse()
    assert a.full and a.dump_outputs == "somewhere"


def test_dump_outputs_writes_float_npy_and_a_fixed_sample(tmp_path, monkeypatch):
    import numpy as np
    import torch

    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    big = torch.arange(5000, dtype=torch.bfloat16).reshape(50, 100)
    arrays = {"small": torch.arange(12).reshape(3, 4), "big": big, "loss": torch.tensor([0.1], dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in arrays}
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "loss.npy", "small.npy"]
    assert got["small"].dtype == np.float32 and got["small"].shape == (3, 4)
    assert np.array_equal(got["small"], np.arange(12, dtype=np.float32).reshape(3, 4))
    assert got["loss"].dtype == np.float64 and got["loss"][0] == 0.1
    # the sample: DUMP_MAX_ELEMS of the array's own elements, in order, the same from run to run
    assert got["big"].dtype == np.float32 and got["big"].shape == (1000,)
    assert np.isin(got["big"], big.float().numpy()).all() and (np.diff(got["big"]) >= 0).all()
    assert np.array_equal(got["big"], np.load(tmp_path / "b" / "big.npy"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) < 64e6


def test_gflop_per_utt_matches_survey():
    sys.argv = ["bench.py"]
    import bench
    a = bench.parse()
    assert abs(bench.gflop_per_utt(a) - 193.87) < 0.05                     # C2
    a.layers, a.d_model, a.heads, a.seq_len, a.batch = 12, 768, 12, 512, 16
    assert abs(bench.gflop_per_utt(a) - 491.68) < 0.05                     # C4
    assert bench.config_tag(a).startswith("C4")
    a.layers, a.d_model, a.heads, a.seq_len, a.batch, a.seconds = 2, 128, 4, 32, 4, 1.0
    assert abs(bench.gflop_per_utt(a) - 14.32) < 0.05                      # C1
