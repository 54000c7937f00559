"""Cost of snapshots next to the env-step they bracket, in one process.

    python tools/snapshot_bench.py [--config cfg3] [--envs 8192] [--substeps 300] [--reps 30] [--warmup 5]

cfg3, 8192 envs, the benchmark's reset states.  Times, with HIP events on the batch stream around the asynchronous (_dev) entry points:
  save_all  - every env into a snapshot of full capacity (one launch of k_snapshot_copy);
  load_all  - the same snapshot back into the batch;
  fork      - env 0 into the 8191 others (hsr_batch_copy_envs_dev: two launches through the scratch snapshot);
and the launches of k_env_step_mf of --reps env-steps of --substeps substeps with fresh random actions (hsr_batch_kernel_times).
Prints one JSON line: the median and the spread of each in milliseconds, the record's size and the bandwidth save_all reaches
(bytes read + bytes written over its median).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--substeps", type=int, default=300)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    from bench import GEOFENCE, sample_inputs
    from hsr_env_amd.compiler import load_config
    from hsr_env_amd.sim import BatchSim
    if not torch.cuda.is_available():
        raise SystemExit("snapshot_bench needs the GPU: a time measured anywhere else says nothing")
    m = load_config(a.config)
    n = a.envs
    dev = torch.device("cuda", 0)
    sim = BatchSim(m, n)
    q0, goal = sample_inputs(m, n, 0, 0)
    sim.reset(qpos0=q0, mocap=goal)
    stream = torch.cuda.ExternalStream(sim.stream_ptr(), device=dev)
    rng = np.random.Generator(np.random.Philox(key=[1, 0]))
    lo, hi = m.act_ctrlrange[:, 0].astype(np.float32), m.act_ctrlrange[:, 1].astype(np.float32)
    d_ctrl = [torch.from_numpy(rng.uniform(lo, hi, (n, m.nu)).astype(np.float32)).to(dev) for _ in range(a.reps + a.warmup)]
    d_obs = torch.empty((n, m.nq + m.nv), dtype=torch.float32, device=dev)
    src = torch.zeros(n - 1, dtype=torch.int32, device=dev)
    dst = torch.arange(1, n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    bid = m.body_id(m.block_body())
    snap = sim.snapshot()
    L, none = sim._L, None

    def must(rc):
        assert rc == 0, L.hsr_last_error()

    def timed(call):
        ms = []
        for k in range(a.reps + a.warmup):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            call()
            t1.record(stream)
            t1.synchronize()
            if k >= a.warmup:
                ms.append(t0.elapsed_time(t1))
        return ms

    for k in range(a.warmup):                       # a state with contacts and caches, as a training run would save it
        sim.step_dev(d_ctrl[k].data_ptr(), a.substeps, bid, GEOFENCE, d_obs.data_ptr(), None, None, None)
    sim.sync()
    times = {"save_all": timed(lambda: must(L.hsr_batch_snapshot_save_dev(sim._b, snap._s, none, none, n))),
             "load_all": timed(lambda: must(L.hsr_batch_snapshot_load_dev(sim._b, snap._s, none, none, n)))}
    sim.set_profiling(2)
    for k in range(a.reps):
        sim.step_dev(d_ctrl[a.warmup + k].data_ptr(), a.substeps, bid, GEOFENCE, d_obs.data_ptr(), None, None, None)
    times["k_env_step_mf"] = list(sim.kernel_times())
    sim.set_profiling(0)
    d_src, d_dst = C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr())
    times["fork_1_to_all"] = timed(lambda: must(L.hsr_batch_copy_envs_dev(sim._b, d_src, d_dst, n - 1)))      # last: it overwrites every env with env 0
    sim.sync()
    words = L.hsr_model_snapshot_record_words(sim._m)
    out = {"config": a.config, "envs": n, "substeps": a.substeps, "reps": a.reps, "unit": "ms", "record_bytes": 4 * words}
    for name, ms in times.items():
        out[name] = {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}
    out["save_all_GBps"] = 2 * 4 * words * n / (out["save_all"]["median"] * 1e-3) / 1e9
    print(json.dumps(out))
    snap.close(); sim.close()


if __name__ == "__main__":
    main()
