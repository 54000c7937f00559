"""Cost of the on-policy rollout next to the env-step it follows, and its GAE and minibatches next to the torch-ops way, in one process.

    python tools/rollout_bench.py [--config cfg3] [--envs 8192] [--substeps 300] [--horizon 32] [--batch 32768]
                                  [--reps 20] [--warmup 3] [--loop-steps 8] [--rounds 3]

cfg3, 8192 envs, 300 substeps per env-step, a horizon of 32 env-steps, minibatches of 32768; blocks and goals from the benchmark's boxes,
episodes of at most 20 env-steps.  HIP events on the batch stream around the asynchronous entry points.  One JSON line:
  (a) stage_close - hsr_rollout_stage_dev + hsr_rollout_close_dev of one env-step, next to k_env_step_mf, the launch of the env-step they
      surround (hsr_batch_kernel_times of the same steps);
  (b) finish - hsr_rollout_finish_dev (GAE and the statistics), and torch_finish - the same on the same tensors with torch ops: a loop over
      t, then mean and std;
  (c) epoch - one epoch of hsr_rollout_minibatch_dev calls, and torch_epoch - torch.randperm and an index_select per field and minibatch
      of the same fields, advantages normalised;
  (d) closed_loop - env-steps/s of control.run on VecHSREnv(auto_reset=True) with and without make_rollout() (the loop with one stages
      constant logp / value rows every step and runs finish + next every `horizon` steps), alternating --rounds times.
Medians with min and max; the two legs of (b) and of (c) alternate.  Needs the GPU.
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
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--lam", type=float, default=0.95)
    ap.add_argument("--limit", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-steps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    from bench import GEOFENCE
    from hsr_env_amd import control
    from hsr_env_amd.compiler import load_config
    from hsr_env_amd.env import GoalSpec
    from hsr_env_amd.episodes import EpisodeSpec
    from hsr_env_amd.sim import BatchSim, RolloutSpec
    from hsr_env_amd.spaces import Box
    if not torch.cuda.is_available():
        raise SystemExit("rollout_bench needs the GPU: a time measured anywhere else says nothing")
    if a.warmup + a.reps > a.horizon:
        raise SystemExit("--warmup + --reps env-steps must fit the horizon: they fill the rollout that (b) and (c) then read")
    m = load_config(a.config)
    n, T, B, od, nu = a.envs, a.horizon, a.batch, m.nq + m.nv, m.nu
    M = T * n
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
    ctrl, obs, final, rew, done, kind = f32(n, nu), f32(n, od), f32(n, od), f32(n), u8(n), u8(n)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    w = torch.randn(od, device=dev, generator=gen) * 0.1               # a linear critic: values of the size of the observations
    # the torch user's store of the same rollout: [T, N] planes and [T, N, .] rows
    t_obs, t_act, t_logp, t_val, t_rew, t_kind, t_vterm = f32(T, n, od), f32(T, n, nu), f32(T, n), f32(T, n), f32(T, n), u8(T, n), f32(T, n)
    _, q, v = sim.get_state()
    obs.copy_(torch.from_numpy(np.concatenate([q, v], axis=1)))
    torch.cuda.synchronize()
    ro = sim.rollout(RolloutSpec(seed=0, env_offset=0, horizon=T, obs_dim=od, gamma=a.gamma, lam=a.lam))
    ro.begin_dev(obs.data_ptr())

    def env_step(k, substeps, timed):
        """One env-step of the loop; returns the milliseconds of stage + close when timed."""
        sim.sample_ctrl_dev(k, ctrl.data_ptr())
        with torch.cuda.stream(stream):
            t_obs[k].copy_(obs); t_act[k].copy_(ctrl)
            torch.mv(obs, w, out=t_val[k])
            torch.sum(ctrl * ctrl, dim=1, out=t_logp[k]); t_logp[k].neg_()
        t0, t1, t2, t3 = (torch.cuda.Event(enable_timing=True) for _ in range(4))
        t0.record(stream)
        ro.stage_dev(ctrl.data_ptr(), t_logp[k].data_ptr(), t_val[k].data_ptr())
        t1.record(stream)
        sim.step_dev(ctrl.data_ptr(), substeps, bid, GEOFENCE, obs.data_ptr(), rew.data_ptr(), done.data_ptr(), None)
        sim.episode_end_dev(obs.data_ptr(), rew.data_ptr(), done.data_ptr(), final.data_ptr(), kind.data_ptr(), None, None)
        t2.record(stream)
        ro.close_dev(rew.data_ptr(), kind.data_ptr(), obs.data_ptr())
        t3.record(stream)
        with torch.cuda.stream(stream):
            t_rew[k].copy_(rew); t_kind[k].copy_(kind)
            torch.mv(final, w, out=t_vterm[k])
        ro.bootstrap_dev(t_vterm[k].data_ptr())
        t3.synchronize()
        return (t0.elapsed_time(t1) + t2.elapsed_time(t3)) if timed else None

    for k in range(a.warmup):
        env_step(k, a.substeps, False)
    sim.set_profiling(2)
    sc_ms = [env_step(a.warmup + k, a.substeps, True) for k in range(a.reps)]
    step_ms = list(sim.kernel_times())
    sim.set_profiling(0)
    for k in range(a.warmup + a.reps, T):          # fill the horizon with short steps: what finish and an epoch cost does not depend on the values
        env_step(k, 5, False)
    last = f32(n)
    with torch.cuda.stream(stream):
        torch.mv(obs, w, out=last)
    sim.sync()

    def timed(call):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        with torch.cuda.stream(stream):
            call()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1)

    # (b) finish is allowed once per filled store (READY at t == T), so between repetitions the store is filled again from the kept rows
    # (next, then T x stage + close + bootstrap), which is not timed
    gamma, gl = np.float32(a.gamma), np.float32(np.float32(a.gamma) * np.float32(a.lam))
    t_adv, t_ret = f32(T, n), f32(T, n)
    t_stats = {}

    def refill():
        ro.next()
        for k in range(T):
            ro.stage_dev(t_act[k].data_ptr(), t_logp[k].data_ptr(), t_val[k].data_ptr())
            ro.close_dev(t_rew[k].data_ptr(), t_kind[k].data_ptr(), (t_obs[k + 1] if k + 1 < T else obs).data_ptr())
            ro.bootstrap_dev(t_vterm[k].data_ptr())

    def device_finish():
        ro.finish_dev(last.data_ptr())

    def torch_finish():
        nxt_v, nxt_a = last, torch.zeros_like(last)
        for t in range(T - 1, -1, -1):
            on, cut = t_kind[t] == 0, t_kind[t] == 2
            nv = torch.where(on, nxt_v, torch.where(cut, t_vterm[t], torch.zeros_like(last)))
            delta = t_rew[t] + float(gamma) * nv - t_val[t]
            torch.add(delta, torch.where(on, nxt_a, torch.zeros_like(last)), alpha=float(gl), out=t_adv[t])
            torch.add(t_adv[t], t_val[t], out=t_ret[t])
            nxt_v, nxt_a = t_val[t], t_adv[t]
        t_stats["mean"] = t_adv.mean()
        t_stats["rstd"] = 1.0 / (t_adv.std(unbiased=False) + 1e-8)

    f_ms, tf_ms = [], []
    for rep in range(a.warmup + a.reps):
        if rep:
            refill()
        f, tf = timed(device_finish), timed(torch_finish)
        if rep >= a.warmup:
            f_ms.append(f); tf_ms.append(tf)
    # the two legs computed the same thing: the torch leg may fuse a product and a sum, so the comparison has a tolerance
    adv_dev = f32(T, n)
    ro.planes_dev(adv_dev.data_ptr(), None)
    sim.sync()
    scale = float(t_adv.abs().max())
    adv_diff = float((adv_dev - t_adv).abs().max()) / max(scale, 1e-30)

    # (c) one epoch of minibatches
    out_t = dict(obs=f32(B, od), action=f32(B, nu), logp=f32(B), value=f32(B), advantage=f32(B), ret=f32(B), index=torch.zeros((B, 2), dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    ptrs = [out_t[k].data_ptr() for k in ("obs", "action", "logp", "value", "advantage", "ret", "index")]
    flat = [x.view(M, -1) if x.dim() == 3 else x.view(M) for x in (t_obs, t_act, t_logp, t_val, t_adv, t_ret)]
    epoch = [0]

    def device_epoch():
        for first in range(0, M, B):
            ro.minibatch_dev(epoch[0], first, min(B, M - first), 1, *ptrs)
        epoch[0] += 1

    def torch_epoch():
        perm = torch.randperm(M, device=dev, generator=gen)
        norm = (flat[4] - t_stats["mean"]) * t_stats["rstd"]
        for first in range(0, M, B):
            idx = perm[first:first + B]
            for k, x in enumerate(flat):
                (norm if k == 4 else x).index_select(0, idx)

    for _ in range(a.warmup):
        timed(device_epoch); timed(torch_epoch)
    e_ms, te_ms = [], []
    for _ in range(a.reps):
        e_ms.append(timed(device_epoch)); te_ms.append(timed(torch_epoch))
    row_bytes = 4 * ((od + nu + 3) // 4 * 4)
    moved = M * (row_bytes + 4 * 4 + 4 * (od + nu + 4 + 2))       # row + four planes read, the outputs written
    ro.close(); sim.close()
    del t_obs, t_act, flat, out_t
    torch.cuda.empty_cache()

    # ---- (d) the closed loop of the driver, with and without a rollout attached
    class RolloutLoopEnv(control.ControlHSREnv):
        """control.run's env with the calls a rollout needs around step(): stage before it, finish + next when the horizon is reached."""
        rollout = None

        def control_agent(self, random_actions=False):
            ro_ = self.rollout
            if ro_ is None:
                return super().control_agent(random_actions)
            action = self.sample_action_dev()
            ro_.stage(action, self._zeros, self._zeros)
            _, _, t, _ = self.step(action)
            ro_.bootstrap(self._zeros)
            if ro_.state()[1] == ro_.horizon:
                ro_.finish(self._zeros)
                ro_.next()
            return t

    env_args = dict(model=m, n_envs=n, steps_per_action=a.substeps, goals=goals, block_space=block_space, auto_reset=True, max_episode_steps=a.limit)
    envs = {"plain": RolloutLoopEnv(**env_args), "with_rollout": RolloutLoopEnv(**env_args)}
    envs["with_rollout"].rollout = envs["with_rollout"].make_rollout(T, gamma=a.gamma, lam=a.lam)
    envs["with_rollout"]._zeros = f32(n)
    torch.cuda.synchronize()
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
    out = {"config": a.config, "envs": n, "substeps": a.substeps, "horizon": T, "batch": B, "reps": a.reps, "row_bytes": row_bytes,
           "stage_close_ms": stat(sc_ms), "k_env_step_mf_ms": stat(step_ms), "finish_ms": stat(f_ms), "torch_finish_ms": stat(tf_ms),
           "finish_vs_torch_max_rel_diff": adv_diff, "epoch_ms": stat(e_ms), "epoch_bytes": moved,
           "epoch_GBps": moved / (float(np.median(e_ms)) * 1e-3) / 1e9, "torch_epoch_ms": stat(te_ms),
           "closed_loop_env_steps_per_s": {name: stat(r) for name, r in rates.items()}}
    plain, with_r = out["closed_loop_env_steps_per_s"]["plain"], out["closed_loop_env_steps_per_s"]["with_rollout"]
    out["closed_loop_cost"] = 1.0 - with_r["median"] / plain["median"]
    out["closed_loop_plain_spread"] = (plain["max"] - plain["min"]) / plain["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
