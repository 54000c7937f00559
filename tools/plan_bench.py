"""Cost of the CEM planner next to the env-steps it drives and to the same work written with torch ops, in one process.

    python tools/plan_bench.py [--config cfg3] [--envs 64] [--samples 64] [--horizon 3] [--iterations 3] [--substeps 300] [--reps 5] [--warmup 2]

cfg3, P = 64 acting envs, K = 64 candidates each (a planning batch of 4096 envs), H = 3 env-steps of 300 substeps, 3 iterations: a plan()
is 9 env-steps of the planning batch.  One JSON line, medians with min and max:
  (a) plan_ms / plans_per_s - a whole CEMPlanner.plan(), host clock (the call ends in a synchronise of the planning stream);
  (b) planner_ms / steps_ms - inside such a call, device events on the planning stream: the planner's own launches (fan-out load, begin,
      sample, accumulate, update, action) against the H x iterations env-steps; planner_share = planner_ms / (planner_ms + steps_ms);
  (c) torch_ms - the stand-in a user would write, on the same stream between the same env-steps: randn draws, clamp, the cost from the
      step's observation rows (the block's position is qpos[7:10]) and done flags, topk, gather, mean and std in float64, the refit; no
      host round trip.  It is timed the same way, with the env-steps left out of the sum.
The two legs alternate.  Needs the GPU.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--horizon", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--substeps", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    from bench import GEOFENCE
    from hsr_env_amd.compiler import load_config
    from hsr_env_amd.env import GoalSpec, VecHSREnv
    from hsr_env_amd.spaces import Box
    if not torch.cuda.is_available():
        raise SystemExit("plan_bench needs the GPU: a time measured anywhere else says nothing")
    m = load_config(a.config)
    P, K, H, I, nu, od = a.envs, a.samples, a.horizon, a.iterations, m.nu, m.nq + m.nv
    N, E = P * K, max(2, K // 8)
    block = m.block_body()
    env = VecHSREnv(model=m, n_envs=P, goals=[GoalSpec(block, Box([-.1, -.2, .422], [.1, .2, .422]), GEOFENCE)], steps_per_action=a.substeps,
                    block_space=Box([-.1, -.2, .422, -np.pi], [.1, .2, .422, np.pi]))
    env.seed(0)
    env.reset()
    planner = env.make_planner(samples=K, horizon=H, iterations=I, elites=E)
    sim, stream, dev = planner.sim, planner.stream, planner.device
    qadr = m.meta["joint_qposadr"][m.names["joint"].index(block + "joint")][0] if (block + "joint") in m.names["joint"] else 7

    def collect(run):
        """run(mark) -> ({kind: ms summed over its segments}, wall ms)."""
        events = []

        def mark(kind):
            e = torch.cuda.Event(enable_timing=True)
            e.record(stream)
            events.append((kind, e))
        t0 = time.perf_counter()
        run(mark)
        stream.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        ms = {"planner": 0.0, "step": 0.0}
        for (_, e0), (kind, e1) in zip(events, events[1:]):
            ms[kind] += e0.elapsed_time(e1)
        return ms, wall

    # the stand-in: the same loop with torch ops where the planner's kernels are
    lo = torch.tensor(np.where(np.abs(m.act_ctrlrange[:, 0]) < 1e30, m.act_ctrlrange[:, 0], -1), dtype=torch.float32, device=dev)
    hi = torch.tensor(np.where(np.abs(m.act_ctrlrange[:, 1]) < 1e30, m.act_ctrlrange[:, 1], 1), dtype=torch.float32, device=dev)
    half = (hi - lo) * 0.5
    t_mean = torch.zeros((P, H, nu), dtype=torch.float32, device=dev).clamp_(lo, hi)
    t_sigma = (0.5 * half).expand(P, H, nu).contiguous()
    t_act = torch.zeros((P, H, nu, K), dtype=torch.float32, device=dev)
    t_ctrl = torch.zeros((N, nu), dtype=torch.float32, device=dev)
    t_obs = torch.zeros((N, od), dtype=torch.float32, device=dev)
    t_done = torch.zeros(N, dtype=torch.uint8, device=dev)
    t_goal = torch.tensor(np.repeat(env._goal_points, K, axis=0), dtype=torch.float32, device=dev)
    gamma = 1.0
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    torch.cuda.synchronize()

    def torch_plan(mark):
        planner.snapshot.save()
        with torch.cuda.stream(stream):
            mark("start")
            t_mean[:, :-1] = t_mean[:, 1:].clone()
            t_sigma.copy_((0.5 * half).expand(P, H, nu))
            for _ in range(I):
                planner.snapshot.load(planner.fan_slot, planner.fan_env, into=sim)
                J = torch.zeros(N, dtype=torch.float32, device=dev)
                g = torch.ones(N, dtype=torch.float32, device=dev)
                alive = torch.ones(N, dtype=torch.bool, device=dev)
                for h in range(H):
                    z = torch.randn((P, K, nu), dtype=torch.float32, device=dev, generator=gen)
                    z[:, 0] = 0
                    x = torch.clamp(t_mean[:, None, h] + t_sigma[:, None, h] * z, lo, hi)
                    t_act[:, h] = x.transpose(1, 2)
                    t_ctrl.copy_(x.reshape(N, nu))
                    mark("planner")
                    sim.step_dev(t_ctrl.data_ptr(), a.substeps, planner.goal_body, planner.geofence, t_obs.data_ptr(), None, t_done.data_ptr(), None)
                    mark("step")
                    d = torch.linalg.vector_norm(t_obs[:, qadr:qadr + 3] - t_goal, dim=1)
                    J = torch.where(alive, J + g * d, J)
                    g = torch.where(alive, g * gamma, g)
                    alive = alive & (t_done == 0)
                Jg = torch.where(torch.isfinite(J), J, torch.full_like(J, float("inf"))).view(P, K)
                idx = Jg.topk(E, dim=1, largest=False).indices
                el = torch.gather(t_act, 3, idx[:, None, None, :].expand(P, H, nu, E)).to(torch.float64)
                mu = el.mean(dim=3)
                sd = ((el - mu[..., None]) ** 2).mean(dim=3).sqrt()
                t_mean.copy_(mu.to(torch.float32))
                t_sigma.copy_(torch.maximum(sd.to(torch.float32), 0.05 * half))
            action = t_mean[:, 0].clone()
            mark("planner")
        return action

    legs = {"fused": lambda mark: planner.plan(mark=mark), "torch": torch_plan}
    for _ in range(a.warmup):
        for run in legs.values():
            collect(run)
    rows = {name: [] for name in legs}
    for _ in range(a.reps):                        # the legs alternate
        for name, run in legs.items():
            rows[name].append(collect(run))
    failed = int(planner.failed.sum())
    planner.close(); env.close()

    stat = lambda x: {"median": float(np.median(x)), "min": float(min(x)), "max": float(max(x))}
    fused, other = rows["fused"], rows["torch"]
    out = {"config": a.config, "envs": P, "samples": K, "horizon": H, "iterations": I, "elites": E, "substeps": a.substeps, "planning_envs": N, "reps": a.reps,
           "plan_ms": stat([w for _, w in fused]), "planner_ms": stat([ms["planner"] for ms, _ in fused]), "steps_ms": stat([ms["step"] for ms, _ in fused]),
           "torch_ms": stat([ms["planner"] for ms, _ in other]), "torch_steps_ms": stat([ms["step"] for ms, _ in other]), "failed": failed}
    out["plans_per_s"] = 1e3 / out["plan_ms"]["median"]
    out["planner_share"] = out["planner_ms"]["median"] / (out["planner_ms"]["median"] + out["steps_ms"]["median"])
    out["planner_over_torch"] = out["planner_ms"]["median"] / out["torch_ms"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
