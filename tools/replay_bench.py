"""Cost of the hindsight replay next to the env-step it follows, and its sampler next to the torch-ops way, in one process.

    python tools/replay_bench.py [--config cfg3] [--envs 8192] [--substeps 300] [--capacity 64] [--batch 32768] [--her 0.8]
                                 [--reps 20] [--warmup 3] [--loop-steps 8] [--rounds 3] [--seq-len 8 --gamma 0.99]

cfg3, 8192 envs, 300 substeps per env-step, a ring of 64 env-steps per env, minibatches of 32768, her_ratio 0.8; blocks and goals from the
benchmark's boxes, episodes of at most 20 env-steps.  HIP events on the batch stream around the asynchronous entry points.  One JSON line:
  (a) record_commit - hsr_replay_record_dev + hsr_replay_commit_dev of one env-step, next to k_env_step_mf, the launch of the env-step
      they follow (hsr_batch_kernel_times of the same steps);
  (b) sample - hsr_replay_sample_dev, and the bytes it moves (row read + outputs written) over its median;
  (c) torch_sample - the same minibatch the way a user would build it today: the same fields in an rl.DeviceReplayBuffer (flat ring of
      T x N items, episode ids kept by torch ops on the reset mask), episode ends and 'future' relabelling in torch ops;
  (d) closed_loop - env-steps/s of control.run on VecHSREnv(auto_reset=True) with and without make_replay(), alternating --rounds times;
  (e) with --seq-len L > 0: seq_sample - hsr_replay_sample_seq_dev, windows of up to L steps and their n-step targets - next to
      torch_seq_sample, the same windows and targets from the same flat ring with torch ops: gather by slot, mask by episode id, the
      n-step sums by cumulative products.
Medians with min and max; (b) and (c) alternate, and so do the two legs of (e).  Needs the GPU.
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
    ap.add_argument("--capacity", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--her", type=float, default=0.8)
    ap.add_argument("--limit", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-steps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seq-len", type=int, default=0, help="0: leave (e) out")
    ap.add_argument("--gamma", type=float, default=0.99)
    a = ap.parse_args()
    import torch
    from bench import GEOFENCE
    from hsr_env_amd import control
    from hsr_env_amd.compiler import load_config
    from hsr_env_amd.env import GoalSpec
    from hsr_env_amd.episodes import EpisodeSpec
    from hsr_env_amd.rl import DeviceReplayBuffer
    from hsr_env_amd.sim import BatchSim, ReplaySeqOut, ReplaySpec
    from hsr_env_amd.spaces import Box
    if not torch.cuda.is_available():
        raise SystemExit("replay_bench needs the GPU: a time measured anywhere else says nothing")
    m = load_config(a.config)
    n, T, B, od, nu = a.envs, a.capacity, a.batch, m.nq + m.nv, m.nu
    dev = torch.device("cuda", 0)
    block = m.block_body()
    bid = m.body_id(block)
    goals = [GoalSpec(block, Box([-.1, -.2, .422], [.1, .2, .422]), GEOFENCE)]
    block_space = Box([-.1, -.2, .422, -np.pi], [.1, .2, .422, np.pi])

    # ---- (a) - (c): one batch driven through the C-ABI's device entry points
    sim = BatchSim(m, n)
    sim.set_episodes(EpisodeSpec.from_env(m, {}, goals, block_space, seed=0, max_episode_steps=a.limit))
    sim.reset_sampled()
    stream = torch.cuda.ExternalStream(sim.stream_ptr(), device=dev)
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)
    ctrl, obs, prev, rew, done, kind = f32(n, nu), f32(n, od), f32(n, od), f32(n), u8(n), u8(n)
    ach, des = f32(n, 3), f32(n, 3)
    _, q, v = sim.get_state()
    obs.copy_(torch.from_numpy(np.concatenate([q, v], axis=1)))
    torch.cuda.synchronize()
    rep = sim.replay(ReplaySpec(seed=0, env_offset=0, capacity_steps=T, obs_dim=od, goal_body=bid, geofence=GEOFENCE))
    rep.commit_dev(obs.data_ptr(), None)
    buf = DeviceReplayBuffer(T * n, device=dev)
    ep_id = torch.ones(n, dtype=torch.int64, device=dev)
    mocap_body = next(i for i, mc in enumerate(m.arrays["body_mocap"]) if mc)

    def env_step(k, substeps, timed):
        """One env-step of the loop; returns the milliseconds of record + commit when timed."""
        sim.sample_ctrl_dev(k, ctrl.data_ptr())
        with torch.cuda.stream(stream):
            prev.copy_(obs)
        sim.step_dev(ctrl.data_ptr(), substeps, bid, GEOFENCE, obs.data_ptr(), rew.data_ptr(), done.data_ptr(), None)
        t0, t1, t2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        t0.record(stream)
        rep.record_dev(ctrl.data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr())
        t1.record(stream)
        # the torch-ops user's bookkeeping of the same step (not timed here): the fields need a visit to the host today
        ach.copy_(torch.from_numpy(sim.body_xpos(bid))); des.copy_(torch.from_numpy(sim.body_xpos(mocap_body)))
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            buf.extend((prev.clone(), ctrl.clone(), obs.clone(), ach.clone(), des.clone(), rew.clone(), done.clone(), ep_id.clone()))
        sim.episode_end_dev(obs.data_ptr(), rew.data_ptr(), done.data_ptr(), None, kind.data_ptr(), None, None)
        t2.record(stream)
        rep.commit_dev(obs.data_ptr(), kind.data_ptr())
        t3 = torch.cuda.Event(enable_timing=True)
        t3.record(stream)
        with torch.cuda.stream(stream):
            ep_id.add_((kind != 0).to(torch.int64))
        t3.synchronize()
        return (t0.elapsed_time(t1) + t2.elapsed_time(t3)) if timed else None

    for k in range(a.warmup):
        env_step(k, a.substeps, False)
    sim.set_profiling(2)
    rc_ms = [env_step(a.warmup + k, a.substeps, True) for k in range(a.reps)]
    step_ms = list(sim.kernel_times())
    sim.set_profiling(0)
    k = a.warmup + a.reps
    while rep.state()[2] < T:                      # top the ring up with short steps: the sampler's cost does not depend on what the rows hold
        env_step(k, 5, False)
        k += 1
    sim.sync()

    out_t = dict(obs=f32(B, od), action=f32(B, nu), next_obs=f32(B, od), goal=f32(B, 3), achieved_next=f32(B, 3), reward=f32(B), done=u8(B),
                 index=torch.zeros((B, 4), dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    ptrs = [out_t[f].data_ptr() for f in ("obs", "action", "next_obs", "goal", "achieved_next", "reward", "done", "index")]
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    b_obs, b_act, b_next, b_ach, b_des, b_rew, b_done, b_id = buf.buffer
    first = buf.pos // n if buf.full else 0        # the flat ring is [T][N]: storage step of age 0
    count = T if buf.full else buf.pos // n
    ages = torch.arange(count, device=dev)

    def torch_indices():
        e = torch.randint(0, n, (B,), device=dev, generator=gen)
        j = torch.randint(0, count, (B,), device=dev, generator=gen)
        relabel = torch.rand(B, device=dev, generator=gen) < a.her
        slots = (first + ages) % T                                              # [count]
        ids = b_id.view(T, n)[slots][:, e]                                      # [count, B] the env's episode ids, oldest first
        own = ids.gather(0, j[None, :])
        run = (ids == own) & (ages[:, None] >= j[None, :])
        j_end = j + run.sum(0) - 1
        j_goal = torch.minimum(j + (torch.rand(B, device=dev, generator=gen) * (j_end - j + 1).float()).long(), j_end)
        return e, j, relabel, j_end, j_goal

    def torch_sample():
        e, j, relabel, j_end, j_goal = torch_indices()
        flat, flat_goal = ((first + j) % T) * n + e, ((first + j_goal) % T) * n + e
        achieved = b_ach[flat]
        goal = torch.where(relabel[:, None], b_ach[flat_goal], b_des[flat])
        reach = (achieved - goal).norm(dim=1) < GEOFENCE
        reward = torch.where(relabel, reach.float(), b_rew[flat])
        done_ = torch.where(relabel, reach, b_done[flat] != 0)
        return b_obs[flat], b_act[flat], b_next[flat], goal, achieved, reward, done_

    draw = [0]

    def device_sample():
        rep.sample_dev(draw[0], B, a.her, *ptrs)
        draw[0] += 1

    def timed(call):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        with torch.cuda.stream(stream):
            call()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1)

    for _ in range(a.warmup):
        timed(device_sample); timed(torch_sample)
    s_ms, t_ms = [], []
    for _ in range(a.reps):
        s_ms.append(timed(device_sample)); t_ms.append(timed(torch_sample))
    row_bytes = 4 * ((2 * od + nu + 10 + 3) // 4 * 4)
    moved = B * (row_bytes + 4 * (2 * od + nu + 3 + 3 + 1 + 4) + 1)

    # ---- (e) windows and n-step targets: the device sampler next to the torch-ops construction, on the same ring
    L, seq = a.seq_len, None
    if L > 0:
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
        seq_t = dict(obs=f32(B, L, od), act=f32(B, L, nu), next_obs=f32(B, L, od), achieved_next=f32(B, L, 3), goal=f32(B, 3), reward=f32(B, L),
                     done=u8(B, L), length=i32(B), nstep=i32(B), nstep_return=f32(B), nstep_discount=f32(B), nstep_obs=f32(B, od), nstep_done=u8(B),
                     index=i32(B, 4))
        torch.cuda.synchronize()
        seq_out = ReplaySeqOut(**{k: v.data_ptr() for k, v in seq_t.items()})
        steps = torch.arange(L, device=dev)
        powers = torch.tensor(a.gamma, dtype=torch.float32, device=dev) ** steps            # gamma^k
        ones = torch.ones((B, 1), dtype=torch.float32, device=dev)

        def device_seq_sample():
            rep.sample_seq_dev(draw[0], B, L, a.her, a.gamma, seq_out)
            draw[0] += 1

        def torch_seq_sample():
            e, j, relabel, j_end, j_goal = torch_indices()
            length = torch.clamp(j_end - j + 1, max=L)
            valid = steps[None, :] < length[:, None]                                    # [B, L]
            age = torch.where(valid, j[:, None] + steps[None, :], j[:, None])
            flat = ((first + age) % T) * n + e[:, None]                                 # [B, L] slots of the window in the flat ring
            flat_goal = ((first + j_goal) % T) * n + e
            mask = valid[:, :, None]
            obs_w, act_w, next_w, ach_w = (torch.where(mask, x[flat], 0.0) for x in (b_obs, b_act, b_next, b_ach))
            goal = torch.where(relabel[:, None], b_ach[flat_goal], b_des[flat[:, 0]])
            reach = (b_ach[flat] - goal[:, None, :]).norm(dim=2) < GEOFENCE
            reward = torch.where(relabel[:, None], reach.float(), b_rew[flat]) * valid
            done_w = torch.where(relabel[:, None], reach, b_done[flat] != 0) & valid
            # step k counts while no earlier step of the window was done: a cumulative product of (1 - done), shifted by one
            alive = torch.cumprod(torch.cat([ones, 1.0 - done_w[:, :-1].float()], dim=1), dim=1) * valid
            m = alive.sum(1).long()
            ret = (alive * powers[None, :] * reward).sum(1)
            last = (m - 1)[:, None]
            return (obs_w, act_w, next_w, ach_w, goal, reward, done_w, length, m, ret, powers[m - 1] * a.gamma, b_next[flat.gather(1, last)[:, 0]],
                    done_w.gather(1, last)[:, 0])

        for _ in range(a.warmup):
            timed(device_seq_sample); timed(torch_seq_sample)
        q_ms, tq_ms = [], []
        for _ in range(a.reps):
            q_ms.append(timed(device_seq_sample)); tq_ms.append(timed(torch_seq_sample))
        seq = (q_ms, tq_ms)
        del seq_t
    rep.close(); sim.close()
    del buf, b_obs, b_act, b_next, b_ach, b_des, b_rew, b_done, b_id
    torch.cuda.empty_cache()

    # ---- (d) the closed loop of the driver, with and without a replay attached
    env_args = dict(model=m, n_envs=n, steps_per_action=a.substeps, goals=goals, block_space=block_space, auto_reset=True, max_episode_steps=a.limit)
    envs = {"plain": control.ControlHSREnv(**env_args), "with_replay": control.ControlHSREnv(**env_args)}
    envs["with_replay"].make_replay(T, her_ratio=a.her)
    for env in envs.values():
        env.reset()

    def loop(env, steps):
        with contextlib.redirect_stdout(io.StringIO()):
            control.run(env, steps, random_actions=True)
        env.sim.sync()

    for env in envs.values():
        loop(env, a.warmup)
    rates = {name: [] for name in envs}
    for _ in range(a.rounds):
        for name, env in envs.items():
            t0 = time.perf_counter()
            loop(env, a.loop_steps)
            rates[name].append(a.loop_steps * n / (time.perf_counter() - t0))
    for env in envs.values():
        env.close()

    stat = lambda x: {"median": float(np.median(x)), "min": float(min(x)), "max": float(max(x))}
    out = {"config": a.config, "envs": n, "substeps": a.substeps, "capacity": T, "batch": B, "her_ratio": a.her, "reps": a.reps, "row_bytes": row_bytes,
           "record_commit_ms": stat(rc_ms), "k_env_step_mf_ms": stat(step_ms), "sample_ms": stat(s_ms), "sample_bytes": moved,
           "sample_GBps": moved / (float(np.median(s_ms)) * 1e-3) / 1e9, "torch_sample_ms": stat(t_ms),
           "closed_loop_env_steps_per_s": {name: stat(r) for name, r in rates.items()}}
    plain, with_r = out["closed_loop_env_steps_per_s"]["plain"], out["closed_loop_env_steps_per_s"]["with_replay"]
    out["closed_loop_cost"] = 1.0 - with_r["median"] / plain["median"]
    out["closed_loop_plain_spread"] = (plain["max"] - plain["min"]) / plain["median"]
    if seq:
        out.update({"seq_len": L, "gamma": a.gamma, "seq_sample_ms": stat(seq[0]), "torch_seq_sample_ms": stat(seq[1])})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
