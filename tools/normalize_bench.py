"""Cost of the running-moments normaliser next to the env-step and to the same work written with torch ops, in one process.

    python tools/normalize_bench.py [--config cfg3] [--envs 8192] [--substeps 300] [--batch 4096] [--reps 20] [--warmup 3] [--calls 20]

cfg3, 8192 envs, 300 substeps per env-step, a 4096-row sample.  HIP events on the batch stream around the asynchronous entry points; the
short calls are timed `--calls` at a time and reported per call.  One JSON line, medians with min and max, in milliseconds:
  (a) k_env_step_mf - the launch of the env-step (hsr_batch_kernel_times of the timed steps);
  (b) observe - what the device loop adds to an env-step: ObsNormalizer.observe of the step's [envs, nq + nv] rows, i.e. the update (two
      passes and the finish: three launches) and the apply into policy_obs (one launch);
  (c) torch_observe - the stand-in a user would write: a finite-row mask, float64 mean and sum of squared deviations of the batch, Chan's
      merge into device tensors, sqrt / reciprocal, and (x - mean) * rstd clamped, all torch ops on the same stream, no host round trip;
  (d) apply_batch - ObsNormalizer.apply_batch of obs, next_obs [batch, nq + nv] and goal, achieved_next [batch, 3] in one launch;
  (e) torch_apply_batch - the same four tensors with sub_ / mul_ / clamp_ in place, from float32 mean and 1 / std vectors made beforehand;
  (f) update_big / torch_update_big - the update alone (three launches) of `--big` = 65 536 rows of the same columns, where every
      workgroup of the second pass adds up the first pass's partials of all 512 tiles, against the stand-in's moments and merge.
The legs alternate.  Needs the GPU.
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
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--big", type=int, default=65536, help="rows of the large update leg")
    ap.add_argument("--limit", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window of the short entry points")
    a = ap.parse_args()
    import torch
    from bench import GEOFENCE
    from hsr_env_amd.compiler import load_config
    from hsr_env_amd.env import GoalSpec
    from hsr_env_amd.episodes import EpisodeSpec
    from hsr_env_amd.normalize import ObsNormalizer, RunningNorm
    from hsr_env_amd.sim import BatchSim
    from hsr_env_amd.spaces import Box
    if not torch.cuda.is_available():
        raise SystemExit("normalize_bench needs the GPU: a time measured anywhere else says nothing")
    m = load_config(a.config)
    n, B, od, nu = a.envs, a.batch, m.nq + m.nv, m.nu
    dev = torch.device("cuda", 0)
    block = m.block_body()
    bid = m.body_id(block)
    goals = [GoalSpec(block, Box([-.1, -.2, .422], [.1, .2, .422]), GEOFENCE)]
    block_space = Box([-.1, -.2, .422, -np.pi], [.1, .2, .422, np.pi])
    sim = BatchSim(m, n)
    sim.set_episodes(EpisodeSpec.from_env(m, {}, goals, block_space, seed=0, max_episode_steps=a.limit))
    sim.reset_sampled()
    stream = torch.cuda.ExternalStream(sim.stream_ptr(), device=dev)
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)
    ctrl, obs, rew, done, kind = f32(n, nu), f32(n, od), f32(n), u8(n), u8(n)
    nz = ObsNormalizer(sim, od)
    eps, clip = nz.obs.eps, nz.obs.clip

    def event():
        e = torch.cuda.Event(enable_timing=True)
        e.record(stream)
        return e

    def env_step(k):
        sim.sample_ctrl_dev(k, ctrl.data_ptr())
        sim.step_dev(ctrl.data_ptr(), a.substeps, bid, GEOFENCE, obs.data_ptr(), rew.data_ptr(), done.data_ptr(), None)
        sim.episode_end_dev(obs.data_ptr(), rew.data_ptr(), done.data_ptr(), None, kind.data_ptr(), None, None)
        sim.sync()

    for k in range(a.warmup):
        env_step(k)
    sim.set_profiling(2)
    for k in range(a.reps):
        env_step(a.warmup + k)
    step_ms = list(sim.kernel_times())
    sim.set_profiling(0)

    # the stand-in's state: device tensors, so that nothing visits the host
    t_count = torch.zeros((), dtype=torch.float64, device=dev)
    t_mean, t_m2 = torch.zeros(od, dtype=torch.float64, device=dev), torch.zeros(od, dtype=torch.float64, device=dev)
    t_policy = f32(n, od)
    zero64 = torch.zeros((), dtype=torch.float64, device=dev)

    def observe():
        nz.observe(obs)

    def torch_observe():
        fin = torch.isfinite(obs).all(dim=1, keepdim=True)
        x = obs.to(torch.float64)
        cnt = fin.sum().to(torch.float64)
        mean_b = torch.where(fin, x, zero64).sum(0) / cnt
        m2_b = torch.where(fin, (x - mean_b) ** 2, zero64).sum(0)
        delta, tot = mean_b - t_mean, t_count + cnt
        t_mean.add_(delta * cnt / tot)
        t_m2.add_(m2_b + delta * delta * t_count * cnt / tot)
        t_count.copy_(tot)
        std = torch.sqrt(torch.clamp(t_m2 / t_count, min=eps * eps))
        torch.clamp((obs - t_mean.to(torch.float32)) * (1.0 / std).to(torch.float32), -clip, clip, out=t_policy)

    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    batch = dict(obs=f32(B, od), next_obs=f32(B, od), goal=f32(B, 3), achieved_next=f32(B, 3))
    for t in batch.values():
        t.copy_(torch.randn(t.shape, device=dev, generator=gen))
    nz.goal.update(batch["goal"])
    torch.cuda.synchronize()

    def apply_batch():
        nz.apply_batch(batch)

    pub = {}

    def torch_apply_batch():         # the float32 vectors are made once, outside the timed calls, as the fused leg's are published beforehand
        for key in ("obs", "next_obs"):
            batch[key].sub_(pub["mean"]).mul_(pub["rstd"]).clamp_(-clip, clip)
        for key in ("goal", "achieved_next"):
            batch[key].sub_(pub["gmean"]).mul_(pub["grstd"]).clamp_(-clip, clip)

    # the update alone at the largest batch the library is meant for, on rows of the step's columns
    big_rows = torch.randn((a.big, od), device=dev, generator=gen)
    torch.cuda.synchronize()
    big_norm = RunningNorm(sim, od)
    big_norm.update(big_rows)          # the partial sums are allocated here, not in a timed call
    b_count = torch.zeros((), dtype=torch.float64, device=dev)
    b_mean, b_m2 = torch.zeros(od, dtype=torch.float64, device=dev), torch.zeros(od, dtype=torch.float64, device=dev)

    def update_big():
        big_norm.update(big_rows)

    def torch_update_big():
        fin = torch.isfinite(big_rows).all(dim=1, keepdim=True)
        x = big_rows.to(torch.float64)
        cnt = fin.sum().to(torch.float64)
        mean_b = torch.where(fin, x, zero64).sum(0) / cnt
        m2_b = torch.where(fin, (x - mean_b) ** 2, zero64).sum(0)
        delta, tot = mean_b - b_mean, b_count + cnt
        b_mean.add_(delta * cnt / tot)
        b_m2.add_(m2_b + delta * delta * b_count * cnt / tot)
        b_count.copy_(tot)

    def timed(call):
        with torch.cuda.stream(stream):
            t0 = event()
            for _ in range(a.calls):
                call()
            t1 = event()
        t1.synchronize()
        return t0.elapsed_time(t1) / a.calls

    names = dict(observe=observe, torch_observe=torch_observe, apply_batch=apply_batch, torch_apply_batch=torch_apply_batch, update_big=update_big,
                 torch_update_big=torch_update_big)
    with torch.cuda.stream(stream):
        torch_observe()
        std = torch.sqrt(torch.clamp(t_m2 / t_count, min=eps * eps))
        pub.update(mean=t_mean.to(torch.float32), rstd=(1.0 / std).to(torch.float32))
        pub.update(gmean=pub["mean"][:3].clone(), grstd=pub["rstd"][:3].clone())
    for _ in range(a.warmup):
        for call in names.values():
            timed(call)
    ms = {name: [] for name in names}
    for _ in range(a.reps):                        # the legs alternate
        for name, call in names.items():
            ms[name].append(timed(call))
    count = nz.obs.count
    big_norm.close(); nz.close(); sim.close()

    stat = lambda x: {"median": float(np.median(x)), "min": float(min(x)), "max": float(max(x))}
    out = {"config": a.config, "envs": n, "substeps": a.substeps, "obs_dim": od, "batch": B, "big": a.big, "reps": a.reps, "calls_per_window": a.calls,
           "k_env_step_mf_ms": stat(step_ms), **{name + "_ms": stat(x) for name, x in ms.items()}, "rows_counted": count}
    out["observe_over_env_step"] = out["observe_ms"]["median"] / out["k_env_step_mf_ms"]["median"]
    out["observe_over_torch"] = out["observe_ms"]["median"] / out["torch_observe_ms"]["median"]
    out["apply_batch_over_torch"] = out["apply_batch_ms"]["median"] / out["torch_apply_batch_ms"]["median"]
    out["update_big_over_torch"] = out["update_big_ms"]["median"] / out["torch_update_big_ms"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
