"""Episodes on the device (include/hsrsim.h: hsr_batch_set_episodes .. hsr_batch_episode_state) against the numpy restatement of
tests/episode_ref.py: the sampler is the stated function bit for bit, a shard draws and computes what the single batch does, the
auto-reset equals the manual loop over the existing entry points, and the Python surface reports episodes as rl.TimeLimit would.

cfg2, 70 envs (more than one wave, not a multiple of 64) and 5 substeps per env-step unless a test says otherwise."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch        # before the library: torch's HIP runtime must be the first one loaded into the process (as in test_rl.py)

import episode_ref as ref
from hsr_env_amd.env import GoalSpec, VecHSREnv
from hsr_env_amd.episodes import EpisodeSpec
from hsr_env_amd.spaces import Box

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
N, SUB, GEOFENCE = 70, 5, 0.05
SEED = 2 ** 40 + 7
BLOCK_START = Box([-.05, -.05, .422, 1, 0, 0, 0], [.05, .05, .422, 1, 0, 0, 0])
GOAL = Box([-.05, -.05, .422], [.05, .05, .422])
BLOCK_SPACE = Box([-.1, -.2, .422, -3.14], [.1, .2, .5, 3.14])
MOCAP_BODY = 1


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits_equal(a, b):
    return np.array_equal(u32(a), u32(b))


def cfg2_spec(m, seed=SEED, offset=0, limit=3):
    return EpisodeSpec.from_env(m, {"block0joint": BLOCK_START}, [GoalSpec("block0", GOAL, GEOFENCE)], None, seed=seed, env_offset=offset,
                                max_episode_steps=limit)


class Dev:
    """The device tensors one batch's loop reads and writes; `host()` waits for the batch and copies them."""

    def __init__(self, sim):
        import torch
        self.sim, self.torch = sim, torch
        n, no, dev = sim.n, sim.nq + sim.nv, torch.device("cuda", 0)
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)
        self.t = dict(ctrl=f32(n, sim.nu), obs=f32(n, no), final=f32(n, no), rew=f32(n), fret=f32(n), done=u8(n), kind=u8(n), mask=u8(n),
                      flen=torch.zeros(n, dtype=torch.int32, device=dev), q=f32(n, sim.nq), g=f32(n, 3))
        torch.cuda.synchronize()

    def p(self, k):
        return self.t[k].data_ptr()

    def put(self, k, a):
        self.sim.sync()
        dtype = {self.torch.float32: np.float32, self.torch.uint8: np.uint8, self.torch.int32: np.int32}[self.t[k].dtype]
        self.t[k].copy_(self.torch.from_numpy(np.ascontiguousarray(a, dtype)))
        self.torch.cuda.synchronize()

    def host(self, *keys):
        self.sim.sync()
        return [self.t[k].cpu().numpy() for k in keys]

    def step(self, goal_body):
        self.sim.step_dev(self.p("ctrl"), SUB, goal_body, GEOFENCE, self.p("obs"), self.p("rew"), self.p("done"), None)

    def episode_end(self):
        self.sim.episode_end_dev(self.p("obs"), self.p("rew"), self.p("done"), self.p("final"), self.p("kind"), self.p("fret"), self.p("flen"))


def state_of(sim):
    t, q, v = sim.get_state()
    return np.concatenate([t[:, None], q, v, sim.get_warmstart(), sim.body_xpos(MOCAP_BODY)], axis=1)


# ------------------------------------------------------------------ 1. sampling is the stated function
def check_block_space(sim, m, n, seed):
    spec = EpisodeSpec.from_env(m, {}, None, BLOCK_SPACE, seed=seed)
    sim.set_episodes(spec)
    sim.reset_sampled()
    q = sim.get_state()[1]
    want, _, half = ref.sample_start(spec, np.arange(n), np.zeros(n, np.uint32))
    quat = np.zeros(m.nq, bool)
    for b, a in enumerate(spec.block_qadr):
        quat[[a + 3, a + 6]] = True
        # device cosf / sinf of the float32 half yaw against float64: a few ulp at 1.0, not the sampler
        assert np.abs(q[:, a + 3] - np.cos(half[:, b].astype(np.float64))).max() < 1e-6
        assert np.abs(q[:, a + 6] - np.sin(half[:, b].astype(np.float64))).max() < 1e-6
        assert np.ptp(q[:, a]) > 0 and np.all(q[:, a:a + 3] >= BLOCK_SPACE.low[:3]) and np.all(q[:, a:a + 3] <= BLOCK_SPACE.high[:3])
    assert bits_equal(q[:, ~quat], want[:, ~quat])              # x, y, z and the two zeros of every block, and every other qpos entry
    assert bits_equal(sim.body_xpos(MOCAP_BODY), np.zeros((n, 3)))


def test_sampling_is_the_stated_function(models):
    from hsr_env_amd.sim import BatchSim
    m = models["cfg2"]
    spec = cfg2_spec(m)
    sim = BatchSim(m, N)
    sim.set_episodes(spec)
    sim.reset_sampled()
    gids = np.arange(N)
    q0, g0, _ = ref.sample_start(spec, gids, np.zeros(N, np.uint32))
    assert bits_equal(sim.get_state()[1], q0) and bits_equal(sim.body_xpos(MOCAP_BODY), g0)
    assert np.ptp(q0[:, 2]) > 0.05 and np.ptp(g0[:, 1]) > 0.05 and np.all(q0[:, :2] == 0)
    index, q, g = np.ones(N, np.uint32), q0.copy(), g0.copy()
    for mask in (gids % 3 == 0, gids % 5 == 0):
        sim.reset_sampled(mask)
        qs, gs, _ = ref.sample_start(spec, gids, index)
        q[mask], g[mask] = qs[mask], gs[mask]
        index[mask] += 1
        assert bits_equal(sim.get_state()[1], q) and bits_equal(sim.body_xpos(MOCAP_BODY), g)
    ei, el, er = sim.episode_state()
    assert np.array_equal(ei, index) and index.min() == 1 and index.max() == 3 and not el.any() and not er.any()
    check_block_space(sim, m, N, SEED)
    sim.close()
    m4 = models["cfg4"]
    sim = BatchSim(m4, 6)
    check_block_space(sim, m4, 6, SEED)
    sim.close()


# ------------------------------------------------------------------ 2. shard invariance
def test_a_shard_draws_and_computes_what_the_single_batch_does(models):
    from hsr_env_amd.sim import BatchSim
    m = models["cfg2"]
    bid = m.body_id("block0")
    parts = [(N, 0), (32, 0), (38, 32)]
    sims = [BatchSim(m, n) for n, _ in parts]
    devs = []
    for sim, (n, off) in zip(sims, parts):
        sim.set_episodes(cfg2_spec(m, offset=off))
        sim.reset_sampled()
        devs.append(Dev(sim))

    def same(get):
        whole, a, b = [get(k) for k in range(3)]
        return np.array_equal(whole, np.concatenate([a, b]))

    assert same(lambda k: u32(state_of(sims[k])))
    resets = 0
    for step in range(6):
        for sim, d in zip(sims, devs):
            sim.sample_ctrl_dev(step, d.p("ctrl"))
            d.step(bid)
            d.episode_end()
        out = [d.host("obs", "final", "rew", "kind", "fret", "flen", "ctrl") for d in devs]
        for j in range(7):
            assert same(lambda k: out[k][j].view(np.uint32 if out[k][j].dtype == np.float32 else out[k][j].dtype)), (step, j)
        assert same(lambda k: u32(state_of(sims[k]))), step
        resets += int((out[0][3] != 0).sum())
    assert resets > N                                           # every env was reset at least once (the limit is 3), many twice
    for sim in sims:
        sim.close()


# ------------------------------------------------------------------ 3. auto-reset equals the manual loop
def test_auto_reset_equals_the_manual_loop_over_the_existing_entry_points(models):
    """Batch A closes every env-step with hsr_batch_episode_end_dev.  Batch B never hears of episodes: the test keeps the books on the host
    (episode_ref.Books), uploads the restatement's samples and the mask done | over, and calls hsr_batch_reset_dev.  SEED was chosen on the
    CPU (OracleBatchSim stepped with the same samples): from the third env-step on every step resets some envs on done, truncates
    others and lets the rest go on."""
    from hsr_env_amd.sim import BatchSim, F_CONTACT
    m = models["cfg2"]
    bid = m.body_id("block0")
    spec = cfg2_spec(m)
    gids = np.arange(N)
    A, B = BatchSim(m, N), BatchSim(m, N)
    dA, dB = Dev(A), Dev(B)
    A.set_episodes(spec)
    A.reset_sampled()
    books = ref.Books(spec, gids)
    mask, q, g, _ = books.begin()
    dB.put("mask", mask); dB.put("q", q); dB.put("g", g)
    B.reset_dev(dB.p("mask"), dB.p("q"), dB.p("g"))

    def compare(step):
        assert bits_equal(state_of(A), state_of(B)), step
        A.forward(); B.forward()
        assert bits_equal(A.get_field(F_CONTACT), B.get_field(F_CONTACT)), step
        assert bits_equal(state_of(A), state_of(B)), step

    compare(-1)
    mixed = 0
    for step in range(8):
        ctrl = ref.sample_ctrl(SEED, gids, step, m.act_ctrlrange)
        dA.put("ctrl", ctrl); dB.put("ctrl", ctrl)
        dA.step(bid); dA.episode_end()
        dB.step(bid)
        obs_b, rew_b, done_b = dB.host("obs", "rew", "done")
        kind, fin_r, fin_l, q, g = books.end(rew_b, done_b)
        sel = kind != 0
        dB.put("mask", sel); dB.put("q", q); dB.put("g", g)
        B.reset_dev(dB.p("mask"), dB.p("q"), dB.p("g"))
        obs_a, final_a, rew_a, done_a, kind_a, fret_a, flen_a = dA.host("obs", "final", "rew", "done", "kind", "fret", "flen")
        assert bits_equal(final_a, obs_b) and bits_equal(rew_a, rew_b) and np.array_equal(done_a, done_b), step
        assert np.array_equal(kind_a, kind) and bits_equal(fret_a, fin_r) and np.array_equal(flen_a, fin_l), step
        want = obs_b.copy()
        want[sel] = np.concatenate([q[sel], np.zeros((int(sel.sum()), m.nv), np.float32)], axis=1)
        assert bits_equal(obs_a, want), step
        ei, el, er = A.episode_state()
        assert np.array_equal(ei, books.index) and np.array_equal(el, books.length) and bits_equal(er, books.ret), step
        compare(step)
        counts = [(kind == 1).sum(), (kind == 2).sum(), (kind == 0).sum()]
        print(f"step {step}: done {counts[0]}, truncated {counts[1]}, going on {counts[2]}")
        mixed += all(c > 0 for c in counts)
    assert mixed >= 1
    A.close(); B.close()


# ------------------------------------------------------------------ 4. actions
def test_sampled_actions_are_the_stated_function(models):
    from hsr_env_amd.sim import BatchSim
    for cfg, offset in (("cfg2", 0), ("cfg3_setxml", 1000)):
        m = models[cfg]
        sim = BatchSim(m, N)
        sim.set_episodes(EpisodeSpec.from_env(m, seed=SEED, env_offset=offset))
        d = Dev(sim)
        cr = m.act_ctrlrange.astype(np.float32)
        free = ~(np.abs(cr) < np.float32(1e30))
        if cfg == "cfg3_setxml":
            assert free[2].all() and free.sum() == 2           # arm_lift_joint's actuator has no ctrlrange in this model
        else:
            assert not free.any()
        lo, hi = np.where(free[:, 0], -1, cr[:, 0]), np.where(free[:, 1], 1, cr[:, 1])
        seen = []
        for step in (0, 1, 2 ** 32 - 1):
            sim.sample_ctrl_dev(step, d.p("ctrl"))
            ctrl, = d.host("ctrl")
            assert bits_equal(ctrl, ref.sample_ctrl(SEED, offset + np.arange(N), step, m.act_ctrlrange)), (cfg, step)
            assert np.all(ctrl >= lo) and np.all(ctrl <= hi) and np.all(np.ptp(ctrl, axis=0) > 0.25 * (hi - lo)), (cfg, step)
            seen.append(ctrl)
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[0], seen[2])
        sim.close()


# ------------------------------------------------------------------ 5. errors
def test_bad_specs_are_refused_and_leave_the_batch_usable(models):
    from hsr_env_amd.sim import BatchSim
    m = models["cfg2"]
    sim = BatchSim(m, N)
    d = Dev(sim)

    def refused(call, word):
        with pytest.raises(AssertionError) as ei:               # HSR_EINVAL (sim._check)
            call()
        assert word in str(ei.value), str(ei.value)

    refused(d.episode_end, "hsr_batch_set_episodes")
    refused(lambda: sim.sample_ctrl_dev(0, d.p("ctrl")), "hsr_batch_set_episodes")
    refused(sim.reset_sampled, "hsr_batch_set_episodes")
    assert sim._L.hsr_batch_set_episodes(sim._b, None) == -1 and b"null spec" in sim._L.hsr_last_error()
    good = cfg2_spec(m)

    def variant(**kw):
        s = cfg2_spec(m)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    lo = good.qpos_lo.copy(); lo[2] = good.qpos_hi[2] + 1
    nan = good.qpos_hi.copy(); nan[0] = np.nan
    ginf = good.goal_hi.copy(); ginf[1] = np.inf
    refused(lambda: sim.set_episodes(variant(qpos_lo=lo)), "lo > hi")
    refused(lambda: sim.set_episodes(variant(qpos_hi=nan)), "not finite")
    refused(lambda: sim.set_episodes(variant(goal_hi=ginf)), "not finite")
    refused(lambda: sim.set_episodes(variant(max_episode_steps=-1)), "max_episode_steps")
    refused(lambda: sim.set_episodes(variant(block_qadr=np.array([3], np.int32))), "free joint")
    refused(lambda: sim.set_episodes(variant(block_qadr=np.array([2, 2], np.int32))), "nblock")
    refused(d.episode_end, "hsr_batch_set_episodes")           # a refused spec does not switch episodes on
    obs, rew, done, ns = sim.step(np.zeros((N, m.nu), np.float32), SUB, m.body_id("block0"), GEOFENCE)
    assert np.all(np.isfinite(obs)) and np.all(ns > 0)
    sim.set_episodes(good)
    sim.reset_sampled()
    sim.set_episodes(good)                                      # twice: the books start again
    assert not sim.episode_state()[0].any()
    sim.reset_sampled()
    d.step(m.body_id("block0")); d.episode_end()
    assert sim.episode_state()[1].max() <= 1
    sim.close()


# ------------------------------------------------------------------ 6. Python surface
def run_env(env, steps, seed):
    env.seed(seed)
    out = [np.array(env.reset())]
    rng = np.random.default_rng(0)
    for _ in range(steps):
        obs, rew, done, info = env.step(rng.uniform(-1, 1, (env.n_envs, env.model.nu)).astype(np.float32))
        out += [np.array(obs), np.array(rew), np.array(done), np.array(info["terminal_observation"]), np.array(info["TimeLimit.truncated"]),
                np.array(info["episode"]["r"]), np.array(info["episode"]["l"])]
    return out


@pytest.mark.parametrize("n", [8, 1])
def test_env_reports_episodes_as_a_time_limit_wrapper_would(models, n):
    m = models["cfg2"]
    no = m.nq + m.nv
    env = VecHSREnv(model=m, n_envs=n, goals=[GoalSpec("block0", GOAL, GEOFENCE)], starts={"block0joint": BLOCK_START}, steps_per_action=SUB,
                    auto_reset=True, max_episode_steps=3)
    env.seed(SEED)
    first = env.reset()
    assert np.shape(first) == ((no,) if n == 1 else (n, no))
    goal0 = np.array(env.goals[0].b)
    assert goal0.shape == ((3,) if n == 1 else (n, 3)) and np.all(goal0 >= GOAL.low) and np.all(goal0 <= GOAL.high)
    n_done = n_trunc = 0
    length = np.zeros(n, int)
    for k in range(7):
        obs, rew, done, info = env.step(np.zeros((n, m.nu), np.float32))
        assert {"terminal_observation", "TimeLimit.truncated", "episode", "log count", "substeps"} <= set(info)
        term, trunc, ep = info["terminal_observation"], info["TimeLimit.truncated"], info["episode"]
        if n == 1:
            assert np.shape(obs) == (no,) and isinstance(rew, float) and isinstance(done, bool) and isinstance(trunc, bool)
            assert np.shape(term) == (no,) and isinstance(ep["r"], float) and isinstance(ep["l"], int)
        else:
            assert obs.shape == (n, no) and rew.shape == (n,) and done.shape == (n,) and done.dtype == bool and trunc.shape == (n,)
            assert term.shape == (n, no) and ep["r"].shape == (n,) and ep["l"].shape == (n,)
        done, trunc, success = np.atleast_1d(done), np.atleast_1d(trunc), np.atleast_1d(info["log count"]["success"])
        assert np.array_equal(done, success | trunc) and not np.any(success & trunc)
        length += 1
        assert np.array_equal(trunc, ~success & (length >= 3))
        assert np.array_equal(np.atleast_1d(ep["l"]), np.where(done, length, 0)) and np.array_equal(np.atleast_1d(ep["r"]), success.astype(np.float32))
        differs = np.any(np.atleast_2d(term) != np.atleast_2d(obs), axis=1)
        assert np.array_equal(differs, done)                    # the returned rows of reset envs are the next episode's first observation
        assert np.all(np.atleast_2d(obs)[done, m.nq:] == 0)
        length[done] = 0
        n_done += int(success.sum()); n_trunc += int(trunc.sum())
    assert n_trunc > 0 and (n == 1 or n_done > 0)
    a, b = run_env(env, 5, 21), run_env(env, 5, 21)
    assert all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))
    c = run_env(env, 5, 22)
    assert not np.array_equal(a[0], c[0])
    env.close()


def test_openai_observations_around_the_reset(models):
    """obs_type='openai': terminal_observation is the openai observation before the reset, the returned rows the one after it - both
    against obs_openai() of a twin batch that steps the same actions and resets the same envs by hand (reset_sampled with a mask)."""
    from hsr_env_amd.sim import BatchSim
    m = models["cfg3"]
    n = 8
    goals = [GoalSpec("block0", GOAL, GEOFENCE)]
    starts = {"block0joint": BLOCK_START}
    env = VecHSREnv(model=m, n_envs=n, goals=goals, starts=starts, steps_per_action=SUB, obs_type="openai", auto_reset=True, max_episode_steps=2)
    env.seed(SEED)
    spec = EpisodeSpec.from_env(m, starts, goals, None, seed=SEED, max_episode_steps=2)
    twin = BatchSim(m, n)
    twin.set_episodes(spec)
    books = ref.Books(spec, np.arange(n))
    first = env.reset()
    twin.reset_sampled(); books.begin()
    assert first.shape == (n, 25) and bits_equal(first, twin.obs_openai())
    resets = 0
    for k in range(4):
        act = ref.sample_ctrl(SEED, np.arange(n), k, m.act_ctrlrange)
        obs, rew, done, info = env.step(act)
        _, rew_t, done_t, _ = twin.step(act, SUB, m.body_id("block0"), GEOFENCE)
        before = twin.obs_openai()
        kind = books.end(rew_t, done_t)[0]
        twin.reset_sampled(kind != 0)
        assert np.array_equal(done, kind != 0) and bits_equal(info["terminal_observation"], before) and bits_equal(obs, twin.obs_openai()), k
        resets += int((kind != 0).sum())
    assert resets >= n
    env.close(); twin.close()


def test_driver_runs_whole_episodes_on_the_device():
    flags = ["--block-space", "(-.1,.1)(-.2,.2)(.422,.422)(-3.14,3.14)", "--steps-per-action=300", "--geofence=.5", "--goal-space", "(-.1,.1)(-.2,.2)(.422,.422)",
             "--use-dof", "slide_x", "--use-dof", "slide_y", "--n-blocks", "1", "--auto-reset", "--max-episode-steps", "4", "--n-envs", "70",
             "--env-steps", "6", "--random-actions"]
    p = subprocess.run([sys.executable, "-m", "hsr_env_amd.control"] + flags, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if "env-steps/s" in l][-1]
    mt = re.fullmatch(r"6 env-steps x 70 envs in ([\d.]+) s -> ([\d.]+) env-steps/s", line.strip())
    assert mt and float(mt.group(2)) > 0, line
