"""Cost of the replay's priorities next to the env-step, to the uniform sampler and to the torch-ops way, in one process.

    python tools/replay_prio_bench.py [--config cfg3] [--envs 8192] [--substeps 300] [--capacity 64] [--batch 4096] [--her 0.8]
                                      [--reps 20] [--warmup 3] [--calls 20]

cfg3, 8192 envs, 300 substeps per env-step, two rings of 64 env-steps per env fed by the same steps - one with priorities, one without -,
minibatches of 4096.  HIP events on the batch stream around the asynchronous entry points; the short calls are timed `--calls` at a time
and reported per call.  One JSON line, medians with min and max, in milliseconds:
  (a) k_env_step_mf - the launch of the env-step (hsr_batch_kernel_times of the timed steps);
  (b) record / record_prio - hsr_replay_record_dev without and with priorities (leaf set + one re-sum launch per stored level);
  (c) sample / sample_prio - hsr_replay_sample_dev and hsr_replay_priority_sample_dev (descent + the same row copy), alternating;
  (d) update_prio - hsr_replay_priority_update_dev of one minibatch's cells;
  (e) torch_draw / torch_update - the stand-in a user would write around the uniform sampler: a float64 cumsum over all T N priorities and a
      searchsorted for the stratified targets; index_put_ of the new priorities.  (It draws cells only - no rows, no relabelling.)
Needs the GPU.
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
    ap.add_argument("--capacity", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--her", type=float, default=0.8)
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
    from hsr_env_amd.sim import BatchSim, PrioritySpec, ReplaySpec
    from hsr_env_amd.spaces import Box
    if not torch.cuda.is_available():
        raise SystemExit("replay_prio_bench needs the GPU: a time measured anywhere else says nothing")
    m = load_config(a.config)
    n, T, B, od, nu = a.envs, a.capacity, a.batch, m.nq + m.nv, m.nu
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
    _, q, v = sim.get_state()
    obs.copy_(torch.from_numpy(np.concatenate([q, v], axis=1)))
    torch.cuda.synchronize()
    spec = ReplaySpec(seed=0, env_offset=0, capacity_steps=T, obs_dim=od, goal_body=bid, geofence=GEOFENCE)
    plain, prio = sim.replay(spec), sim.replay(spec)
    prio.priority_enable(PrioritySpec(1.0, 1e-6, 1e6, B))
    for rep in (plain, prio):
        rep.commit_dev(obs.data_ptr(), None)

    def event():
        e = torch.cuda.Event(enable_timing=True)
        e.record(stream)
        return e

    def env_step(k, substeps):
        """One env-step feeding both rings; returns the milliseconds of (record, record with priorities)."""
        sim.sample_ctrl_dev(k, ctrl.data_ptr())
        sim.step_dev(ctrl.data_ptr(), substeps, bid, GEOFENCE, obs.data_ptr(), rew.data_ptr(), done.data_ptr(), None)
        order = (plain, prio) if k % 2 == 0 else (prio, plain)          # alternate who goes first
        ms = {}
        for rep in order:
            t0 = event()
            rep.record_dev(ctrl.data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr())
            t1 = event()
            ms[rep] = (t0, t1)
        sim.episode_end_dev(obs.data_ptr(), rew.data_ptr(), done.data_ptr(), None, kind.data_ptr(), None, None)
        for rep in (plain, prio):
            rep.commit_dev(obs.data_ptr(), kind.data_ptr())
        sim.sync()
        return ms[plain][0].elapsed_time(ms[plain][1]), ms[prio][0].elapsed_time(ms[prio][1])

    for k in range(a.warmup):
        env_step(k, a.substeps)
    sim.set_profiling(2)
    rec = [env_step(a.warmup + k, a.substeps) for k in range(a.reps)]
    step_ms = list(sim.kernel_times())
    sim.set_profiling(0)
    k = a.warmup + a.reps
    while plain.state()[2] < T:                    # top the rings up with short steps: no cost below depends on what the rows hold
        env_step(k, 5)
        k += 1

    out_t = dict(obs=f32(B, od), action=f32(B, nu), next_obs=f32(B, od), goal=f32(B, 3), achieved_next=f32(B, 3), reward=f32(B), done=u8(B),
                 index=torch.zeros((B, 4), dtype=torch.int32, device=dev))
    prob, new_prio = f32(B), f32(B)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    new_prio.copy_(10.0 ** (torch.rand(B, device=dev, generator=gen) * 6 - 4))
    leaves = f32(T, n)
    torch.cuda.synchronize()
    ptrs = [out_t[f].data_ptr() for f in ("obs", "action", "next_obs", "goal", "achieved_next", "reward", "done", "index")]
    draw = [0]
    token = prio.priority_state()[0]

    def sample():
        plain.sample_dev(draw[0], B, a.her, *ptrs)
        draw[0] += 1

    def sample_prio():
        prio.priority_sample_dev(draw[0], B, a.her, *ptrs, prob.data_ptr())
        draw[0] += 1

    def update_prio():
        prio.priority_update_dev(token, B, out_t["index"].data_ptr(), new_prio.data_ptr())

    # the stand-in: the priorities as a flat float32 tensor, as a user would keep them next to the uniform ring
    prio.priority_read_dev(leaves.data_ptr())
    sim.sync()
    flat = leaves.view(-1).clone()
    strata = torch.arange(B, device=dev, dtype=torch.float64)

    def torch_draw():
        csum = torch.cumsum(flat.to(torch.float64), 0)
        u = (strata + torch.rand(B, device=dev, dtype=torch.float64, generator=gen)) / B * csum[-1]
        cell = torch.searchsorted(csum, u, right=True).clamp_(max=flat.numel() - 1)
        return cell, flat[cell] / csum[-1]

    cells = [None]

    def torch_update():
        flat.index_put_((cells[0],), new_prio)

    def timed(call):
        t0 = event()
        with torch.cuda.stream(stream):
            for _ in range(a.calls):
                call()
        t1 = event()
        t1.synchronize()
        return t0.elapsed_time(t1) / a.calls

    with torch.cuda.stream(stream):
        cells[0] = torch_draw()[0]
    names = dict(sample=sample, sample_prio=sample_prio, update_prio=update_prio, torch_draw=torch_draw, torch_update=torch_update)
    for _ in range(a.warmup):
        for call in names.values():
            timed(call)
    ms = {name: [] for name in names}
    for _ in range(a.reps):                        # the legs alternate
        for name, call in names.items():
            ms[name].append(timed(call))
    pushed, total, p_new = prio.priority_state()
    plain.close(); prio.close(); sim.close()

    stat = lambda x: {"median": float(np.median(x)), "min": float(min(x)), "max": float(max(x))}
    out = {"config": a.config, "envs": n, "substeps": a.substeps, "capacity": T, "leaves": T * n, "batch": B, "her_ratio": a.her, "reps": a.reps,
           "calls_per_window": a.calls, "k_env_step_mf_ms": stat(step_ms), "record_ms": stat([r[0] for r in rec]), "record_prio_ms": stat([r[1] for r in rec]),
           **{name + "_ms": stat(x) for name, x in ms.items()}, "total": total, "p_new": p_new}
    out["record_prio_extra_over_env_step"] = (out["record_prio_ms"]["median"] - out["record_ms"]["median"]) / out["k_env_step_mf_ms"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
