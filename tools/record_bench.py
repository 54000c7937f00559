"""Cost of recording: env-step time with in-step frame capture off and on, and the time to render the captured frames.

    python tools/record_bench.py [--config cfg3] [--envs 8192] [--substeps 300] [--every 20] [--steps 10] [--rounds 5] [--size 500]

The batch steps bench.py's inputs (sample_inputs, a fresh random action per env-step, the bench's goal and geofence).  Three capture
settings alternate round by round in one process - off, one env, 64 envs (every --every substeps) - each timed over --steps env-steps
with device events on the batch stream after a warm-up step; reported are the median ms per env-step of each setting and its spread
over the rounds.  Then render_frames_dev of the last step's frames (rgb, --size x --size) is timed for both capture settings.  Prints
one JSON line.
"""
from __future__ import annotations

import argparse
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
    ap.add_argument("--every", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", type=int, default=500)
    a = ap.parse_args()
    import torch
    from bench import GEOFENCE, sample_inputs
    from hsr_env_amd.compiler import load_config
    from hsr_env_amd.render import default_camera
    from hsr_env_amd.sim import BatchSim
    m = load_config(a.config)
    n = a.envs
    dev = torch.device("cuda", 0)
    sim = BatchSim(m, n)
    q0, goal = sample_inputs(m, n, 0, 0)
    sim.reset(qpos0=q0, mocap=goal)
    stream = torch.cuda.ExternalStream(sim.stream_ptr(), device=dev)
    gb = m.body_id(m.block_body())
    lo = torch.tensor(m.act_ctrlrange[:, 0], dtype=torch.float32, device=dev)
    hi = torch.tensor(m.act_ctrlrange[:, 1], dtype=torch.float32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    ctrls = [lo + (hi - lo) * torch.rand((n, m.nu), generator=gen, device=dev) for _ in range(a.steps)]
    obs = torch.empty((n, m.nq + m.nv), device=dev)
    rew = torch.empty(n, device=dev)
    done = torch.empty(n, dtype=torch.uint8, device=dev)
    ns = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    settings = {"off": [], "1_env": [0], "64_envs": list(range(0, n, max(1, n // 64)))[:64]}

    def run(ids):
        sim.set_capture(ids, a.every if ids else 0)
        sim.step_dev(ctrls[0].data_ptr(), a.substeps, gb, GEOFENCE, obs.data_ptr(), rew.data_ptr(), done.data_ptr(), ns.data_ptr())   # warm-up
        sim.sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for c in ctrls:
            sim.step_dev(c.data_ptr(), a.substeps, gb, GEOFENCE, obs.data_ptr(), rew.data_ptr(), done.data_ptr(), ns.data_ptr())
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / len(ctrls)

    times = {k: [] for k in settings}
    for _ in range(a.rounds):
        for k, ids in settings.items():
            times[k].append(run(ids))
    res = {"config": a.config, "envs": n, "substeps": a.substeps, "every": a.every, "env_steps_per_round": a.steps, "rounds": a.rounds,
           "step_ms": {k: {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in times.items()}}
    off = np.median(times["off"])
    res["step_overhead_pct"] = {k: round(100 * (np.median(v) / off - 1), 2) for k, v in times.items() if k != "off"}
    cam = default_camera(m)
    res["render_frames_ms"] = {}
    for k in ("1_env", "64_envs"):
        run(settings[k])
        rows = sim.capture_rows()
        img = torch.empty((len(settings[k]), rows, a.size, a.size, 3), dtype=torch.uint8, device=dev)
        render = lambda: sim.render_frames_dev(a.size, a.size, cam, rgb=img)
        render()
        sim.sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(5):
            render()
        e1.record(stream)
        e1.synchronize()
        counts = sim.capture_counts()
        res["render_frames_ms"][k] = {"ms": round(e0.elapsed_time(e1) / 5, 3), "images": int(counts.sum()) + len(counts),
                                      "size": a.size}
    sim.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
