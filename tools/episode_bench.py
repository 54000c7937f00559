"""Closed-loop rate of whole episodes: env-steps/s of three loops over the same workload, in one process.

    python tools/episode_bench.py [--config cfg3] [--envs 8192] [--substeps 300] [--limit 20] [--steps 40] [--warmup 5] [--rounds 3]

cfg3, 8192 envs, 300 substeps per env-step, random actions, episodes of at most 20 env-steps; blocks and goals drawn from the benchmark's
boxes, geofence 0.05.
  (a) host   - the driver loop as it was before episodes ran on the device: `if done: env.reset(mask)` with the numpy sampler of
               VecHSREnv.reset, rl.TimeLimit counting on the host, actions from action_space.sample;
  (b) replay - the loop bench.py times: actions and reset states sampled and uploaded before the timed region, step_dev + reset_dev
               (done flags only: it has no time limit, nothing a trainer could use - the ceiling);
  (c) device - control.run on VecHSREnv(auto_reset=True, max_episode_steps=20) with actions from sample_ctrl_dev.
The loops alternate round by round; each round times --steps env-steps after --warmup, between synchronisations.  Prints one JSON line
with the median rate of each loop and its spread over the rounds.
"""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--substeps", type=int, default=300)
    ap.add_argument("--limit", type=int, default=20)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    from bench import GEOFENCE, sample_inputs
    from hsr_env_amd import control
    from hsr_env_amd.compiler import load_config
    from hsr_env_amd.env import GoalSpec
    from hsr_env_amd.rl import TimeLimit
    from hsr_env_amd.sim import BatchSim
    from hsr_env_amd.spaces import Box
    if not torch.cuda.is_available():
        raise SystemExit("episode_bench needs the GPU: a rate measured anywhere else says nothing")
    m = load_config(a.config)
    n, K, W = a.envs, a.steps, a.warmup
    dev = torch.device("cuda", 0)
    block = m.block_body()
    env_args = dict(model=m, n_envs=n, steps_per_action=a.substeps, goals=[GoalSpec(block, Box([-.1, -.2, .422], [.1, .2, .422]), GEOFENCE)],
                    block_space=Box([-.1, -.2, .422, -np.pi], [.1, .2, .422, np.pi]))

    # (a) the host loop
    env_a = TimeLimit(control.ControlHSREnv(**env_args), a.limit)
    env_a.reset()
    state_a = {"done": np.zeros(n, bool)}

    def loop_host(steps):
        done = state_a["done"]
        for _ in range(steps):
            if np.any(done):
                env_a.reset(mask=done)
            _, _, done, _ = env_a.step(env_a.action_space.sample(n, rng=env_a.np_random))
        state_a["done"] = done
        env_a.sim.sync()

    # (b) bench.py's loop: everything the timed region consumes is resident before it starts
    sim_b = BatchSim(m, n)
    q0, goal = sample_inputs(m, n, 0, 0)
    sim_b.reset(qpos0=q0, mocap=goal)
    rng = np.random.Generator(np.random.Philox(key=[1, 0]))
    lo, hi = m.act_ctrlrange[:, 0].astype(np.float32), m.act_ctrlrange[:, 1].astype(np.float32)
    slots = K + W
    d_ctrl = [torch.from_numpy(rng.uniform(lo, hi, (n, m.nu)).astype(np.float32)).to(dev) for _ in range(slots)]
    resets = [sample_inputs(m, n, 2 + k, 0) for k in range(slots)]
    d_rq = [torch.from_numpy(r[0]).to(dev) for r in resets]
    d_rg = [torch.from_numpy(r[1]).to(dev) for r in resets]
    d_obs = torch.empty((n, m.nq + m.nv), dtype=torch.float32, device=dev)
    d_rew = torch.empty(n, dtype=torch.float32, device=dev)
    d_done = torch.empty(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    bid = m.body_id(block)
    pos_b = [0]

    def loop_replay(steps):
        for _ in range(steps):
            k = pos_b[0] % slots
            pos_b[0] += 1
            sim_b.step_dev(d_ctrl[k].data_ptr(), a.substeps, bid, GEOFENCE, d_obs.data_ptr(), d_rew.data_ptr(), d_done.data_ptr(), None)
            sim_b.reset_dev(None, d_rq[k].data_ptr(), d_rg[k].data_ptr())
        sim_b.sync()

    # (c) episodes on the device, through the driver
    env_c = control.ControlHSREnv(auto_reset=True, max_episode_steps=a.limit, **env_args)
    env_c.reset()

    def loop_device(steps):
        with contextlib.redirect_stdout(io.StringIO()):
            control.run(env_c, steps, random_actions=True)
        env_c.sim.sync()

    loops = {"host": loop_host, "replay": loop_replay, "device": loop_device}
    rates = {k: [] for k in loops}
    for f in loops.values():
        f(W)
    for _ in range(a.rounds):
        for name, f in loops.items():
            t0 = time.perf_counter()
            f(K)
            rates[name].append(K * n / (time.perf_counter() - t0))
    out = {"config": a.config, "envs": n, "substeps": a.substeps, "limit": a.limit, "steps": K, "rounds": a.rounds, "unit": "env-steps/s"}
    for name, r in rates.items():
        out[name] = {"median": float(np.median(r)), "min": float(min(r)), "max": float(max(r))}
    print(json.dumps(out))
    env_a.close(); env_c.close(); sim_b.close()


if __name__ == "__main__":
    main()
