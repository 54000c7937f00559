"""The N > 1 path of bench.py with two REAL ranks on the one GPU a test box has (round-3 verdict item 6): the ranks are fresh
child processes started by bench.py's own launcher (`--gpus 2` as a plain command), each drives its own 8192-env shard on cuda:0, and the
all-gather goes through gloo on host copies (`--rehearse-on-one-gpu`: RCCL refuses two ranks on one device).  The number it prints is not a
result; what is checked is the control flow a multi-GPU run takes and that sharding reproduces the single-process run env for env.
The file name puts it first in the session: the test process itself has then not touched the GPU when it starts the children."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def _bench(args, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py")] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["cfg3", "cfg4"])
def test_two_ranks_on_one_gpu_reproduce_the_single_process_shards(tmp_path, cfg):
    """cfg4 (the per-GPU shard of BASELINE configs 4 / 5: three blocks, 4096 two-env tasks on 2048 resident workgroups) takes the work queue, the gather
    and the reset of finished envs in one process pair."""
    two = tmp_path / "two.npy"
    common = ["--config", cfg, "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-capacity"]
    line = _bench(["--gpus", "2", "--rehearse-on-one-gpu", "--full"] + common + ["--dump-step", str(two)])
    assert cfg in line["config"]["workload"] and line["config"]["gather_mode"] == "in line (closed loop)"
    assert line["n_gpus"] == 2 and line["steps"] == 2 and line["warmup"] == 1 and line["scaling"] == "weak"
    assert line["config"]["global_envs"] == 16384 and line["config"]["envs_per_gpu"] == 8192
    assert "gloo (rehearsal)" in line["config"]["parallelism"] and "2 ranks" in line["config"]["parallelism"]
    assert line["value"] > 0 and line["config"]["bad_envs"] == 0
    assert line["roofline"]["launches_timed"] == 2 and (cfg != "cfg3" or line["roofline"]["traffic_source"])
    g = np.load(two)
    nobs = g.shape[1] - 2
    assert g.shape[0] == 16384 and np.isfinite(g).all()
    # each rank's rows of the gathered buffer == a one-rank run of the same global env ids (inputs are keyed by the shard's offset);
    # these runs are plain ones (no --full), and their --dump-outputs arrays are the columns of the --dump-step buffer
    for r in (0, 1):
        one = tmp_path / f"one{r}.npy"
        outs = tmp_path / f"outputs{r}"
        l1 = _bench(["--gpus", "1"] + common + ["--env-offset", str(8192 * r), "--dump-step", str(one), "--dump-outputs", str(outs)])
        assert l1["config"]["gather_mode"] is None
        assert l1["n_gpus"] == 1 and l1["config"]["global_envs"] == 8192
        assert l1["steps"] == 2 and l1["ms_per_step"] > 0 and "roofline" not in l1 and "cpu_baseline" not in l1
        o = np.load(one)
        assert o.shape == (8192, nobs + 2)
        assert np.array_equal(g[8192 * r:8192 * (r + 1)], o), f"rank {r}'s shard of the gathered step differs from the single-process run of the same envs"
        d = {k: np.load(outs / f"{k}.npy") for k in ("obs", "reward", "done", "nsteps")}
        assert all(a.dtype == np.float32 for a in d.values()) and not (outs / "env_index.npy").exists()
        assert np.array_equal(d["obs"], o[:, :nobs]) and np.array_equal(d["reward"], o[:, nobs]) and np.array_equal(d["done"], o[:, nobs + 1])
        assert d["nsteps"].shape == (8192,) and ((d["nsteps"] >= 0) & (d["nsteps"] <= 300)).all()
