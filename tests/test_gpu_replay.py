"""Hindsight replay on the device (include/hsrsim.h: hsr_batch_replay_create .. hsr_replay_sample_dev) against the numpy restatement of
tests/replay_ref.py: the ring holds what the loop produced, the sampler is the stated function bit for bit, the relabelled reward is the
env's own goal test, goals stay inside their episode, a shard draws its own samples, calls out of order are refused without a trace, and
the Python surface feeds the ring from VecHSREnv.step.

Main shape: cfg2 with the episode spec of test_gpu_episodes.py (goal box = start box: successes and failures both occur), 70 envs (two
waves, the second partial), 5 substeps, a ring of 7 steps (not a power of two; it wraps), episodes of at most 3 steps, 12 env-steps of
device-sampled actions, minibatches of 193.  obs_dim 17 and nu 2 give rows of 46 words padded to 48."""
import ctypes as C

import numpy as np
import pytest
import torch        # before the library: torch's HIP runtime must be the first one loaded into the process (as in test_gpu_episodes.py)

import replay_ref as ref
from hsr_env_amd.env import GoalSpec, VecHSREnv
from hsr_env_amd.episodes import EpisodeSpec
from hsr_env_amd.sim import ReplaySpec
from test_gpu_episodes import BLOCK_START, GEOFENCE, GOAL, MOCAP_BODY, SEED, cfg2_spec

pytestmark = pytest.mark.gpu
N, SUB, T, LIMIT, STEPS, B = 70, 5, 7, 3, 12, 193
RSEED = 2 ** 35 + 12345             # the replay's own seed
FIELDS = ("obs", "action", "next_obs", "goal", "achieved_next", "reward", "done", "index")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Loop:
    """One batch, the replays fed from it, the restatement fed from per-step downloads, and the host's own history of the steps."""

    def __init__(self, sim, goal_body, sub, capacity, offsets=(0,), seed=RSEED, obs_dim=None):
        self.sim, self.goal_body, self.sub = sim, goal_body, sub
        n, self.od = sim.n, sim.nq + sim.nv if obs_dim is None else obs_dim
        dev = torch.device("cuda", 0)
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)
        self.t = dict(ctrl=f32(n, sim.nu), obs=f32(n, self.od), final=f32(n, self.od), rew=f32(n), done=u8(n), kind=u8(n))
        self.out = {}
        torch.cuda.synchronize()
        spec = lambda off: ReplaySpec(seed=seed, env_offset=off, capacity_steps=capacity, obs_dim=self.od, goal_body=goal_body, geofence=GEOFENCE)
        self.reps = [sim.replay(spec(off)) for off in offsets]
        self.rings = [ref.Ring(n, capacity, self.od, sim.nu, GEOFENCE, seed=seed, env_offset=off) for off in offsets]
        self.history = []              # per env-step: dict of host rows
        self.step_count = 0

    def p(self, k):
        return self.t[k].data_ptr()

    def host(self, *keys):
        self.sim.sync()
        return [self.t[k].cpu().numpy() for k in keys]

    def begin(self):
        """The first observation: every env opens an episode with it."""
        _, q, v = self.sim.get_state()
        self.sim.sync()
        self.t["obs"].copy_(torch.from_numpy(np.concatenate([q, v], axis=1)))
        torch.cuda.synchronize()
        for rep, ring in zip(self.reps, self.rings):
            rep.commit_dev(self.p("obs"), None)
            ring.commit(self.host("obs")[0])

    def step(self):
        sim = self.sim
        sim.sample_ctrl_dev(self.step_count, self.p("ctrl"))
        before, ctrl = self.host("obs", "ctrl")
        sim.step_dev(self.p("ctrl"), self.sub, self.goal_body, GEOFENCE, self.p("obs"), self.p("rew"), self.p("done"), None)
        for rep in self.reps:
            rep.record_dev(self.p("ctrl"), self.p("obs"), self.p("rew"), self.p("done"))
        final, rew, done = self.host("obs", "rew", "done")
        achieved, desired = sim.body_xpos(self.goal_body), sim.body_xpos(MOCAP_BODY)      # between the step and the episode end
        sim.episode_end_dev(self.p("obs"), self.p("rew"), self.p("done"), self.p("final"), self.p("kind"), None, None)
        for rep in self.reps:
            rep.commit_dev(self.p("obs"), self.p("kind"))
        after, kind = self.host("obs", "kind")
        self.history.append(dict(obs=before, action=ctrl, next_obs=final, reward=rew, done=done, achieved_next=achieved, desired=desired, kind=kind))
        for ring in self.rings:
            ring.record(ctrl, final, rew, done, achieved, desired)
            ring.commit(after, kind)
        self.step_count += 1

    def sample(self, which, draw, batch, her):
        """Minibatch `draw` of replay `which` as host arrays."""
        if batch not in self.out:
            dev = torch.device("cuda", 0)
            f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
            self.out[batch] = dict(obs=f32(batch, self.od), action=f32(batch, self.sim.nu), next_obs=f32(batch, self.od), goal=f32(batch, 3),
                                   achieved_next=f32(batch, 3), reward=f32(batch), done=torch.zeros(batch, dtype=torch.uint8, device=dev),
                                   index=torch.zeros((batch, 4), dtype=torch.int32, device=dev))
            torch.cuda.synchronize()
        o = self.out[batch]
        self.reps[which].sample_dev(draw, batch, her, *[o[k].data_ptr() for k in FIELDS])
        self.sim.sync()
        return {k: o[k].cpu().numpy() for k in FIELDS}

    def close(self):
        for rep in self.reps:
            rep.close()
        self.sim.close()


@pytest.fixture(scope="module")
def run(models):
    """The 12-step loop, run once: her_ratio = 0 minibatches and the books after steps 3, 7 and 12, and the minibatches the other tests read
    taken at the end."""
    from hsr_env_amd.sim import BatchSim
    m = models["cfg2"]
    sim = BatchSim(m, N)
    sim.set_episodes(cfg2_spec(m, limit=LIMIT))
    sim.reset_sampled()
    loop = Loop(sim, m.body_id("block0"), SUB, T, offsets=(0, 70, 0))
    loop.begin()
    marks = {}
    for k in range(1, STEPS + 1):
        loop.step()
        if k in (3, 7, 12):
            marks[k] = dict(batch=loop.sample(0, 100 + k, B, 0.0), state=loop.reps[0].state(), want_state=(loop.rings[0].count, loop.rings[0].head_slot, loop.rings[0].pushed),
                            steps=len(loop.history))
    end = {(her, draw): loop.sample(0, draw, B, her) for her in (0.0, 0.5, 1.0) for draw in (0, 1)}
    again = loop.sample(0, 1, B, 0.5)
    future = loop.sample(0, 9, 4096, 1.0)
    shards = [loop.sample(w, 5, B, 0.5) for w in range(3)]
    data = dict(loop=loop, ring=loop.rings[0], marks=marks, end=end, again=again, future=future, shards=shards, model=m)
    yield data
    loop.close()


def step_of_slot(slot, steps, capacity):
    """The env-step (0-based) a slot holds after `steps` steps."""
    last = steps - 1
    return last - (last - slot) % capacity


def test_ring_holds_what_the_loop_produced(run):
    assert ref.row_words(17, 2) == (46, 48)
    for k, mark in run["marks"].items():
        assert mark["state"] == mark["want_state"] == (min(k, T), k % T, k), (k, mark["state"])
        out, hist = mark["batch"], run["loop"].history
        e, slot = out["index"][:, 0], out["index"][:, 1]
        assert np.all(out["index"][:, 2] == -1) and not out["index"][:, 3].any()
        assert np.all((0 <= e) & (e < N) & (0 <= slot) & (slot < min(k, T)))
        step = step_of_slot(slot, mark["steps"], T)
        assert step.min() >= max(0, k - T) and step.max() == k - 1 and len(set(zip(e.tolist(), slot.tolist()))) > 100
        for name, src in (("obs", "obs"), ("action", "action"), ("next_obs", "next_obs"), ("reward", "reward"), ("achieved_next", "achieved_next"),
                          ("goal", "desired")):
            want = np.stack([hist[s][src][env] for s, env in zip(step, e)])
            assert same(out[name], want), (k, name)
        assert np.array_equal(out["done"], np.array([hist[s]["done"][env] for s, env in zip(step, e)], np.uint8))


def test_sampler_is_the_stated_function(run):
    ring = run["ring"]
    for (her, draw), out in run["end"].items():
        want = ring.sample(draw, B, her)
        for name in FIELDS:
            assert same(out[name], want[name]), (her, draw, name)
    assert run["end"][(0.5, 0)]["index"][:, 3].any() and not run["end"][(0.5, 0)]["index"][:, 3].all()
    for name in FIELDS:
        assert same(run["again"][name], run["end"][(0.5, 1)][name]), name                  # the same draw twice: the same bytes
    assert not same(run["end"][(0.5, 0)]["index"], run["end"][(0.5, 1)]["index"])          # another draw: other samples


def test_relabelled_reward_is_the_env_s_own_goal_test(run):
    """What the sampler recomputes for a relabelled goal is what the env-step computed for the real one: for every stored transition whose
    distance |achieved_next - desired| is further than 1e-6 from the geofence, (distance < geofence) equals the stored reward and done.
    (Within 1e-6 the float32 distance of the step - other summation order, fused multiply-adds - may fall on the other side.)"""
    ring = run["ring"]
    dist = np.sqrt(np.sum((ring.achieved.astype(np.float64) - ring.desired.astype(np.float64)) ** 2, axis=-1))
    clear = np.abs(dist - GEOFENCE) > 1e-6
    print(f"{(~clear).sum()} of {clear.size} stored transitions lie within 1e-6 of the geofence; {int((ring.reward != 0).sum())} successes")
    assert (~clear).mean() <= 0.05
    reach = dist < GEOFENCE
    assert np.array_equal(reach[clear], ring.reward[clear] != 0) and np.array_equal(reach[clear], ring.done[clear] != 0)
    assert np.array_equal(ref.within(ring.achieved, ring.desired, GEOFENCE)[clear], reach[clear])      # the restatement's float32 test agrees
    assert (ring.reward[clear] != 0).sum() >= 5 and (ring.reward[clear] == 0).sum() >= 5
    # and the relabelled samples of the device carry exactly that test on their new goal
    out = run["future"]
    d = np.sqrt(np.sum((out["achieved_next"].astype(np.float64) - out["goal"].astype(np.float64)) ** 2, axis=-1))
    far = np.abs(d - GEOFENCE) > 1e-6
    assert np.array_equal((d < GEOFENCE)[far], out["reward"][far] != 0) and np.array_equal(out["done"], (out["reward"] != 0).astype(np.uint8))
    assert np.all((out["reward"] == 0) | (out["reward"] == 1))


def test_future_goals_stay_inside_their_episode(run):
    """her_ratio = 1, B = 4096: every goal slot carries the episode id of its transition and a step at or after it, and the goal is that
    slot's achieved_next bit for bit.  Episodes of all lengths 1..3 occur AS THE RING HOLDS THEM - runs of one episode id per env, some cut
    by the ring's oldest edge or still open at its newest - and the samples fall into runs of each length.  (Counted over the whole loop,
    complete episodes have the lengths 1 and 3 only: with 5 substeps per env-step the block moves about a micrometre, so an episode
    succeeds on its first step or runs into the limit of 3.)"""
    ring, out = run["ring"], run["future"]
    e, slot, gslot, rel = out["index"].T
    assert rel.all() and np.all((0 <= gslot) & (gslot < T))
    assert np.array_equal(ring.ep_id[gslot, e], ring.ep_id[slot, e])
    assert np.all(ring.ep_step[gslot, e] >= ring.ep_step[slot, e])
    assert same(out["goal"], ring.achieved[gslot, e])
    assert (gslot != slot).any() and (gslot == slot).any()
    # the replay's counters are the host's own count of the loop's resets: an episode id per reset, a step per env-step
    kinds = np.stack([h["kind"] for h in run["loop"].history])
    ids, steps, lengths = np.ones(N, np.int64), np.zeros(N, np.int64), []
    for s, kind in enumerate(kinds):
        sl = s % T
        if s >= STEPS - T:
            assert np.array_equal(ring.ep_id[sl], ids) and np.array_equal(ring.ep_step[sl], steps)
        lengths += (steps[kind != 0] + 1).tolist()
        ids, steps = np.where(kind != 0, ids + 1, ids), np.where(kind != 0, 0, steps + 1)
    print(f"lengths of the complete episodes of the loop: {sorted(set(lengths))}")
    by_age = ring.ep_id[ring.slot(np.arange(T))].astype(np.int64)              # [age, env]
    run_len = (by_age[:, None, :] == by_age[None, :, :]).sum(0)                # [age, env]: steps of that step's episode the ring holds
    assert set(np.unique(run_len).tolist()) == {1, 2, 3}, np.unique(run_len)
    age = (slot - ring.slot(0)) % T
    assert set(np.unique(run_len[age, e]).tolist()) == {1, 2, 3}
    assert max(lengths) == LIMIT and min(lengths) == 1


def test_a_shard_draws_its_own_samples(run):
    at0, at70, at0_again = run["shards"]
    assert not same(at0["index"], at70["index"])
    for name in FIELDS:
        assert same(at0[name], at0_again[name]), name
    want = run["loop"].rings[1].sample(5, B, 0.5)
    for name in FIELDS:
        assert same(at70[name], want[name]), name


def test_order_and_arguments_are_checked(models):
    from hsr_env_amd.sim import BatchSim
    m = models["cfg2"]
    bid = m.body_id("block0")
    sim = BatchSim(m, 9)
    sim.set_episodes(cfg2_spec(m, limit=LIMIT))
    sim.reset_sampled()
    L = sim._L
    # ---- create
    ok = dict(seed=1, env_offset=0, capacity_steps=3, obs_dim=17, goal_body=bid, geofence=GEOFENCE)
    for bad in (dict(capacity_steps=0), dict(capacity_steps=-2), dict(obs_dim=0), dict(obs_dim=-1), dict(goal_body=MOCAP_BODY), dict(goal_body=-1),
                dict(goal_body=m.nbody), dict(geofence=0.0), dict(geofence=-1.0), dict(geofence=float("nan")), dict(geofence=float("inf"))):
        with pytest.raises(AssertionError):
            sim.replay(ReplaySpec(**{**ok, **bad}))
    handle = C.c_void_p()
    assert L.hsr_batch_replay_create(sim._b, None, C.byref(handle)) == -1 and L.hsr_batch_replay_create(sim._b, C.byref(ReplaySpec(**ok)), None) == -1
    assert L.hsr_batch_replay_create(None, C.byref(ReplaySpec(**ok)), C.byref(handle)) == -1 and not handle.value
    sim.set_goals([(bid, MOCAP_BODY, 0.5)])
    with pytest.raises(AssertionError, match="extra goal terms"):
        sim.replay(ReplaySpec(**ok))
    sim.set_goals([])
    # ---- protocol; after each refused call the ring is what it was (seen through a her_ratio = 0 minibatch)
    loop = Loop(sim, bid, SUB, 3, seed=1)
    rep, ring = loop.reps[0], loop.rings[0]

    def refuse(call, *args):
        with pytest.raises(AssertionError):
            call(*args)

    rec = (loop.p("ctrl"), loop.p("obs"), loop.p("rew"), loop.p("done"))
    refuse(rep.record_dev, *rec)                               # record before commit
    refuse(rep.sample_dev, 0, 4, 0.5)                          # empty
    assert rep.state() == (0, 0, 0)
    loop.begin()
    refuse(rep.sample_dev, 0, 4, 0.5)                          # committed, still empty
    loop.step(); loop.step()
    sim.sample_ctrl_dev(2, loop.p("ctrl"))
    sim.step_dev(loop.p("ctrl"), SUB, bid, GEOFENCE, loop.p("obs"), loop.p("rew"), loop.p("done"), None)
    rep.record_dev(*rec)
    refuse(rep.record_dev, *rec)                               # two records
    refuse(rep.sample_dev, 0, 4, 0.5)                          # pending
    assert rep.state() == (2, 2, 2)
    final, rew, done, ctrl = loop.host("obs", "rew", "done", "ctrl")
    ach, des = sim.body_xpos(bid), sim.body_xpos(MOCAP_BODY)
    sim.episode_end_dev(loop.p("obs"), loop.p("rew"), loop.p("done"), None, loop.p("kind"), None, None)
    rep.commit_dev(loop.p("obs"), loop.p("kind"))
    after, kind = loop.host("obs", "kind")
    ring.record(ctrl, final, rew, done, ach, des); ring.commit(after, kind)
    assert rep.state() == (3, 0, 3)
    base = loop.sample(0, 3, 64, 0.0)
    for her in (-0.01, 1.01, float("nan"), float("inf")):
        refuse(rep.sample_dev, 0, 4, her)
    refuse(rep.sample_dev, 0, 0, 0.5)
    refuse(rep.sample_dev, 0, -1, 0.5)
    refuse(rep.commit_dev, None, None)                         # no observation
    assert rep.state() == (3, 0, 3)
    got, want = loop.sample(0, 3, 64, 0.0), ring.sample(3, 64, 0.0)
    for name in FIELDS:
        assert same(got[name], base[name]), name               # the refused calls left no trace: the same bytes as before them,
        assert same(got[name], want[name]), name               # and the ring is the one the valid calls alone built
    # extra goal terms set after the replay was made: record refuses, and goes on once they are cleared
    sim.set_goals([(bid, MOCAP_BODY, 0.5)])
    refuse(rep.record_dev, *rec)
    sim.set_goals([])
    loop.step()
    assert rep.state() == (3, 1, 4)
    loop.close()


def test_edges(models):
    from hsr_env_amd.sim import BatchSim
    m2, m3 = models["cfg2"], models["cfg3"]
    # ---- one env, one slot, one sample
    sim = BatchSim(m2, 1)
    sim.set_episodes(cfg2_spec(m2, limit=LIMIT))
    sim.reset_sampled()
    loop = Loop(sim, m2.body_id("block0"), SUB, 1)
    loop.begin()
    for _ in range(3):
        loop.step()
        for her in (0.0, 1.0):
            got, want = loop.sample(0, 7, 1, her), loop.rings[0].sample(7, 1, her)
            for name in FIELDS:
                assert same(got[name], want[name]), name
            assert got["index"][0, :2].tolist() == [0, 0]
    assert loop.reps[0].state() == (1, 0, 3)
    # ---- clear, then reuse
    loop.reps[0].clear(); loop.rings[0].clear()
    assert loop.reps[0].state() == (0, 0, 0)
    with pytest.raises(AssertionError):
        loop.reps[0].sample_dev(0, 1, 0.5)
    with pytest.raises(AssertionError):
        loop.reps[0].record_dev(loop.p("ctrl"), loop.p("obs"), None, None)
    for rep, ring in zip(loop.reps, loop.rings):
        rep.commit_dev(loop.p("obs"), None); ring.commit(loop.host("obs")[0])
    loop.step()
    got, want = loop.sample(0, 1, 1, 1.0), loop.rings[0].sample(1, 1, 1.0)
    for name in FIELDS:
        assert same(got[name], want[name]), name
    assert loop.rings[0].ep_id[0, 0] == 1                      # the counters started again
    # ---- the batch goes first: the handle refuses everything but its own destruction
    rep = loop.reps[0]
    sim.close()
    for call in (rep.state, rep.clear, lambda: rep.sample_dev(0, 1, 0.5), lambda: rep.commit_dev(loop.p("obs"), None)):
        with pytest.raises(AssertionError, match="destroyed"):
            call()
    rep.close()
    rep.close()
    # ---- cfg3: rows of 71 words padded to 72, 65 envs (one lane past a wave), the ring wraps once
    assert ref.row_words(27, 7) == (71, 72)
    sim = BatchSim(m3, 65)
    sim.set_episodes(EpisodeSpec.from_env(m3, {"block0joint": BLOCK_START}, [GoalSpec("block0", GOAL, GEOFENCE)], None, seed=SEED, max_episode_steps=2))
    sim.reset_sampled()
    loop = Loop(sim, m3.body_id("block0"), SUB, 3)
    loop.begin()
    for _ in range(4):
        loop.step()
    assert loop.reps[0].state() == (3, 1, 4)
    for her, draw in ((0.0, 0), (0.8, 1), (1.0, 2)):
        got, want = loop.sample(0, draw, 64, her), loop.rings[0].sample(draw, 64, her)
        for name in FIELDS:
            assert same(got[name], want[name]), (her, name)
    # reward / done NULL: the flag the step latched
    sim.sample_ctrl_dev(4, loop.p("ctrl"))
    sim.step_dev(loop.p("ctrl"), SUB, loop.goal_body, GEOFENCE, loop.p("obs"), loop.p("rew"), loop.p("done"), None)
    loop.reps[0].record_dev(loop.p("ctrl"), loop.p("obs"), None, None)
    final, rew, done, ctrl = loop.host("obs", "rew", "done", "ctrl")
    loop.rings[0].record(ctrl, final, rew, done, sim.body_xpos(loop.goal_body), sim.body_xpos(MOCAP_BODY))
    loop.reps[0].commit_dev(loop.p("obs"), None); loop.rings[0].commit(final, None)
    got, want = loop.sample(0, 3, 64, 0.0), loop.rings[0].sample(3, 64, 0.0)
    for name in FIELDS:
        assert same(got[name], want[name]), name
    loop.close()


def test_create_and_destroy_return_the_device_memory(models):
    """Free device memory (hipMemGetInfo) around six create / destroy cycles on a live batch, and six more where the batch goes first, as
    test_gpu_snapshot.py::test_destroying_a_batch_frees_its_snapshots_and_the_fork_scratch does it: other users of the device can only add
    noise to single cycles, so the SMALLEST loss is compared with half of one ring (2048 envs x 64 steps x 72 words: 38 MB), and the live
    replay must be seen to hold at least its ring."""
    from hsr_env_amd.sim import BatchSim
    m = models["cfg3"]
    n, cap = 2048, 64
    ring = n * cap * ref.row_words(m.nq + m.nv, m.nu)[1] * 4
    spec = ReplaySpec(seed=0, env_offset=0, capacity_steps=cap, obs_dim=m.nq + m.nv, goal_body=m.body_id("block0"), geofence=GEOFENCE)
    sim = BatchSim(m, n)
    lost, held = [], []
    for _ in range(6):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        rep = sim.replay(spec)
        held.append(free0 - torch.cuda.mem_get_info()[0])
        rep.close()
        lost.append(free0 - torch.cuda.mem_get_info()[0])
    sim.close()
    for _ in range(6):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        sim = BatchSim(m, n)
        rep = sim.replay(spec)                                 # never closed by hand before the batch: the batch's to release
        sim.close()
        rep.close()                                            # the handle alone by now
        lost.append(free0 - torch.cuda.mem_get_info()[0])
    print(f"free device memory lost per cycle: {lost} bytes, held by a live replay: {held} bytes; one ring: {ring} bytes")
    assert max(held) >= ring, (held, ring)
    assert min(lost[:6]) < ring // 2 and min(lost[6:]) < ring // 2, (lost, ring)


def test_env_surface(models):
    m = models["cfg2"]
    kw = dict(model=m, goals=[GoalSpec("block0", GOAL, GEOFENCE)], starts={"block0joint": BLOCK_START}, steps_per_action=SUB, n_envs=N)
    rng = np.random.default_rng(5)
    lo, hi = m.act_ctrlrange[:, 0], m.act_ctrlrange[:, 1]
    actions = rng.uniform(np.where(np.abs(lo) < 1e29, lo, -1), np.where(np.abs(hi) < 1e29, hi, 1), (8, N, m.nu)).astype(np.float32)

    def rollout(with_replay):
        env = VecHSREnv(auto_reset=True, max_episode_steps=LIMIT, **kw)
        env.seed(SEED)
        replay = env.make_replay(T) if with_replay else None
        acted_on, results = [env.reset().copy()], []
        for a in actions:
            obs, rew, done, info = env.step(a)
            results.append((obs.copy(), rew.copy(), done.copy(), info["terminal_observation"].copy()))
            acted_on.append(obs.copy())
        return env, replay, acted_on, results

    env, replay, acted_on, results = rollout(True)
    assert len(replay) == T * N and replay.state() == (T, 8 % T, 8)
    out = replay.sample(64)
    env.sim.sync()
    od, dev = m.nq + m.nv, torch.device("cuda", 0)
    shapes = dict(obs=((64, od), torch.float32), action=((64, m.nu), torch.float32), next_obs=((64, od), torch.float32), goal=((64, 3), torch.float32),
                  achieved_next=((64, 3), torch.float32), reward=((64,), torch.float32), done=((64,), torch.uint8), index=((64, 4), torch.int32))
    assert set(out) == set(shapes)
    for k, (shape, dtype) in shapes.items():
        assert tuple(out[k].shape) == shape and out[k].dtype == dtype and out[k].device == dev, k
    host = {k: v.cpu().numpy() for k, v in out.items()}
    e, slot = host["index"][:, 0], host["index"][:, 1]
    step = step_of_slot(slot, 8, T)
    assert same(host["obs"], np.stack([acted_on[s][env_] for s, env_ in zip(step, e)]))
    assert same(host["next_obs"], np.stack([results[s][3][env_] for s, env_ in zip(step, e)]))
    assert same(host["action"], np.stack([actions[s][env_] for s, env_ in zip(step, e)]))
    assert host["index"][:, 3].any()                           # her_ratio 0.8 by default
    first = replay.sample(64)["index"].cpu().numpy()
    assert not np.array_equal(first, host["index"])            # the draw counter advances
    # fork clears the ring: a ring of past transitions cannot follow a jump
    env.fork(0, 1)
    assert len(replay) == 0
    env.step(actions[0])
    assert replay.state() == (1, 1, 1)
    env.close()
    plain, none, _, plain_results = rollout(False)
    assert none is None
    for (o, r, d, t), (o2, r2, d2, t2) in zip(results, plain_results):
        assert same(o, o2) and same(r, r2) and np.array_equal(d, d2) and same(t, t2)          # the replay changes no result
    plain.close()
    with pytest.raises(ValueError, match="auto_reset"):
        VecHSREnv(**kw).make_replay(T)
    with pytest.raises(NotImplementedError, match="point goal"):
        VecHSREnv(auto_reset=True, **{**kw, "goals": None}).make_replay(T)


def test_env_surface_with_the_openai_observation(models):
    """Rows are the 25-float observation, taken on the device before the reset (terminal) and after it (the next episode's first)."""
    m = models["cfg3"]
    env = VecHSREnv(model=m, goals=[GoalSpec("block0", GOAL, GEOFENCE)], starts={"block0joint": BLOCK_START}, steps_per_action=SUB, n_envs=5,
                    obs_type="openai", auto_reset=True, max_episode_steps=2)
    replay = env.make_replay(4, her_ratio=0.5)
    acted_on, terminal = [env.reset().copy()], []
    rng = np.random.default_rng(6)
    for _ in range(3):
        obs, _, _, info = env.step(rng.uniform(-1, 1, (5, m.nu)).astype(np.float32))
        acted_on.append(obs.copy()); terminal.append(info["terminal_observation"].copy())
    out = {k: v for k, v in replay.sample(32).items()}
    env.sim.sync()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    assert host["obs"].shape == (32, 25)
    e, slot = host["index"][:, 0], host["index"][:, 1]
    assert same(host["obs"], np.stack([acted_on[s][i] for s, i in zip(slot, e)]))
    assert same(host["next_obs"], np.stack([terminal[s][i] for s, i in zip(slot, e)]))
    # object_pos of the terminal observation is the achieved goal: the same pose through another kernel (the last bit may differ)
    assert np.allclose(host["achieved_next"], host["next_obs"][:, 3:6], rtol=0, atol=1e-6)
    env.close()
