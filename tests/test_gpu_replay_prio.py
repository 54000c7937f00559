"""Prioritised replay on the device (include/hsrsim.h: hsr_replay_priority_*) against the numpy restatement of tests/replay_prio_ref.py,
bit for bit: the leaves, the total, p_new, the cells drawn, prob and every row of a minibatch, through updates with duplicates, skipped
and stale rows, through records that wrap the ring, for single steps and for windows; the uniform sampler stays what it was; refused
calls leave no trace; and the Python surface draws a cell as often as the restatement says.

Shape: cfg2, 70 envs (two waves, the second partial), minibatches of 193.  The rings are filled by commit / record with fabricated
tensors - no env-step runs, so achieved and desired goals are the resting poses of the batch.  Two rings: T = 7 gives 490 leaves (not a
multiple of 64; two stored levels), T = 67 gives 4690 leaves (three stored levels, the last node of the first stored level partial)."""
import numpy as np
import pytest
import torch        # before the library: torch's HIP runtime must be the first one loaded into the process (as in test_gpu_episodes.py)

import replay_prio_ref as pr
import replay_seq_ref as seq
from hsr_env_amd.env import GoalSpec, VecHSREnv
from hsr_env_amd.sim import PrioritySpec, ReplaySeqOut, ReplaySpec
from test_gpu_episodes import BLOCK_START, GEOFENCE, GOAL, MOCAP_BODY, cfg2_spec
from test_gpu_replay import FIELDS, RSEED, B, N, same
from test_gpu_replay_seq import shapes

pytestmark = pytest.mark.gpu
MAX_BATCH = 256
HER, GAMMA = 0.5, 0.9
DEV = torch.device("cuda", 0)


class Pair:
    """Replays of one batch with priorities, fed with the same fabricated transitions, and their restatement."""

    def __init__(self, sim, goal_body, T, p=(1.0, 1e-6, 1e6), copies=1, seed=RSEED, enable=True, rng=0):
        self.sim, self.T, self.od, self.rng = sim, T, sim.nq + sim.nv, np.random.default_rng(rng)
        spec = ReplaySpec(seed=seed, env_offset=0, capacity_steps=T, obs_dim=self.od, goal_body=goal_body, geofence=GEOFENCE)
        self.reps = [sim.replay(spec) for _ in range(copies)]
        if enable:
            for rep in self.reps:
                rep.priority_enable(PrioritySpec(*p, MAX_BATCH))
        self.ring = pr.PrioRing(sim.n, T, self.od, sim.nu, GEOFENCE, seed=seed, p_init=p[0], p_min=p[1], p_max=p[2], max_batch=MAX_BATCH)
        self.achieved, self.desired = sim.body_xpos(goal_body), sim.body_xpos(MOCAP_BODY)
        self.keep = []

    def dev(self, a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        torch.cuda.synchronize()
        self.keep.append(t)
        return t

    def commit(self, first=False):
        n = self.sim.n
        obs = self.rng.standard_normal((n, self.od)).astype(np.float32)
        mask = None if first else (self.rng.random(n) < 0.3).astype(np.uint8)
        d_obs, d_mask = self.dev(obs), None if first else self.dev(mask)
        for rep in self.reps:
            rep.commit_dev(d_obs.data_ptr(), None if first else d_mask.data_ptr())
        self.ring.commit(obs, mask)

    def record(self):
        n, f = self.sim.n, lambda *s: self.rng.standard_normal(s).astype(np.float32)
        ctrl, nxt, rew, done = f(n, self.sim.nu), f(n, self.od), f(n), (self.rng.random(n) < 0.2).astype(np.uint8)
        t = [self.dev(a) for a in (ctrl, nxt, rew, done)]
        for rep in self.reps:
            rep.record_dev(*[x.data_ptr() for x in t])
        self.ring.record(ctrl, nxt, rew, done, self.achieved, self.desired)

    def push(self, steps):
        if self.ring.state == pr.EMPTY:
            self.commit(first=True)
        for _ in range(steps):
            self.record()
            self.commit()
        self.sim.sync()
        self.keep.clear()

    def leaves(self, which=0):
        t = torch.zeros((self.T, self.sim.n), dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        self.reps[which].priority_read_dev(t.data_ptr())
        self.sim.sync()
        return t.cpu().numpy()

    def sample(self, draw, batch=B, her=HER, which=0, uniform=False):
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=DEV)
        o = dict(obs=f32(batch, self.od), action=f32(batch, self.sim.nu), next_obs=f32(batch, self.od), goal=f32(batch, 3), achieved_next=f32(batch, 3),
                 reward=f32(batch), done=torch.zeros(batch, dtype=torch.uint8, device=DEV), index=torch.full((batch, 4), -7, dtype=torch.int32, device=DEV),
                 prob=torch.full((batch,), -1.0, dtype=torch.float32, device=DEV))
        torch.cuda.synchronize()
        ptr = [o[k].data_ptr() for k in FIELDS]
        if uniform:
            self.reps[which].sample_dev(draw, batch, her, *ptr)
        else:
            self.reps[which].priority_sample_dev(draw, batch, her, *ptr, o["prob"].data_ptr())
        self.sim.sync()
        return {k: v.cpu().numpy() for k, v in o.items()}

    def sample_seq(self, draw, L, batch=B, her=HER, which=0):
        o = {k: torch.zeros(shape, dtype=dtype, device=DEV) for k, (shape, dtype) in shapes(batch, L, self.od, self.sim.nu).items()}
        prob = torch.full((batch,), -1.0, dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        out = ReplaySeqOut(**{"act" if k == "action" else k: v.data_ptr() for k, v in o.items()})
        self.reps[which].priority_sample_seq_dev(draw, batch, L, her, GAMMA, out, prob.data_ptr())
        self.sim.sync()
        got = {k: v.cpu().numpy() for k, v in o.items()}
        got["prob"] = prob.cpu().numpy()
        return got

    def update(self, token, index, prio, which=None, mirror=True):
        d_index, d_prio = self.dev(np.asarray(index, np.int32)), self.dev(np.asarray(prio, np.float32))
        for rep in self.reps if which is None else [self.reps[which]]:
            rep.priority_update_dev(token, len(prio), d_index.data_ptr(), d_prio.data_ptr())
        self.sim.sync()
        if mirror:
            self.ring.update(token, index, prio)

    def check(self, where, draws=(0, 1)):
        """Leaves, total, p_new and whole minibatches against the restatement; total against a rebuild from the device's own leaves."""
        ring = self.ring
        for w, rep in enumerate(self.reps):
            leaves = self.leaves(w)
            pushed, total, p_new = rep.priority_state()
            assert same(leaves, ring.leaves), (where, w)
            assert pushed == ring.pushed and total == ring.total and np.float32(p_new) == ring.p_new, (where, w, pushed, total, p_new)
            assert total == float(pr.build_tree(leaves)[-1][0]), (where, w)
        for draw in draws:
            got, want = self.sample(draw), ring.prio_sample(draw, B, HER)
            for name in FIELDS + ("prob",):
                assert same(got[name], want[name]), (where, draw, name)
            e, slot = got["index"][:, 0], got["index"][:, 1]
            assert np.all(ring.leaves[slot, e] > 0) and np.all(got["prob"] > 0), (where, draw)

    def close(self):
        for rep in self.reps:
            rep.close()


@pytest.fixture(scope="module")
def sim(models):
    from hsr_env_amd.sim import BatchSim
    m = models["cfg2"]
    s = BatchSim(m, N)
    s.set_episodes(cfg2_spec(m, limit=3))
    s.reset_sampled()
    s.sync()
    yield s
    s.close()


@pytest.fixture(scope="module")
def bid(models):
    return models["cfg2"].body_id("block0")


def odd_rows(pair, rng, base_index):
    """An update batch on top of a sample's index: priorities over eight decades, every row once more with another value (duplicates),
    rows out of range, rows of cells no record has reached, and NaN, negative, zero and huge values."""
    n, T = pair.sim.n, pair.T
    index = np.concatenate([base_index[:100], base_index[:100][::-1]])
    prio = (10.0 ** rng.uniform(-7, 1, len(index))).astype(np.float32)
    extra = np.array([[n, 0, 0, 0], [-1, 0, 0, 0], [0, T, 0, 0], [0, -1, 0, 0], [2 ** 31 - 1, 2 ** 31 - 1, 0, 0], [-2 ** 31, -2 ** 31, 0, 0]], np.int64)
    empty = np.array([[e, s, 0, 0] for s in range(T) if pr.newest_record_of_slot(pair.ring.pushed, T, s) is None for e in (0, n - 1)][:8], np.int64).reshape(-1, 4)
    special = np.array([[e, base_index[0, 1], 0, 0] for e in (3, 4, 5, 6, 66, 66)], np.int64)
    index = np.concatenate([index, extra, empty, special])
    prio = np.concatenate([prio, np.full(len(extra) + len(empty), 3.0, np.float32), np.array([np.nan, -2.0, 0.0, 1e38, 0.25, 0.5], np.float32)])
    assert len(prio) == len(index) <= MAX_BATCH
    return index.astype(np.int32), prio.astype(np.float32)


@pytest.mark.parametrize("T", [7, 67])
def test_bit_exact_through_updates_and_wraps(sim, bid, T):
    """Two replays fed alike: the second takes every update batch in reversed row order."""
    pair = Pair(sim, bid, T, copies=2, rng=T)
    rng = np.random.default_rng(100 + T)
    part = T // 2
    pair.push(part)
    pair.check("partly filled")

    def update_both_ways(where, token):
        index, prio = odd_rows(pair, rng, pair.sample(2)["index"])
        pair.update(token, index, prio, which=0)
        pair.update(token, index[::-1], prio[::-1], which=1, mirror=False)
        assert same(pair.leaves(0), pair.leaves(1)), where
        pair.check(where)

    token = pair.ring.pushed
    update_both_ways("partly filled, updated", token)
    assert pair.ring.p_new > 1                                  # an update stored more than p_init: new transitions enter with it
    # stale tokens: one record later the slot it wrote is newer than the token, the rest is live; T records later nothing is
    pair.push(1)
    pair.check("one record later")
    rows = np.array([[5, part, 0, 0], [5, part - 1, 0, 0]], np.int32)
    pair.update(token, rows, np.array([0.125, 0.125], np.float32))
    assert pair.ring.leaves[part, 5] == pair.ring.p_new and pair.ring.leaves[part - 1, 5] == np.float32(0.125)
    pair.check("stale by one record")
    pair.push(T - part - 1)
    assert pair.ring.count == T and pair.ring.pushed == T
    pair.check("full")
    update_both_ways("full, updated", pair.ring.pushed)
    pair.push(part + 1)
    pair.check("wrapped")
    before = pair.ring.leaves.copy()
    index, prio = odd_rows(pair, rng, pair.sample(2)["index"])
    pair.update(token, index, prio)                             # T records after the token: every row is stale
    assert same(pair.ring.leaves, before)
    pair.check("stale by T records")
    update_both_ways("wrapped, updated", pair.ring.pushed)
    # after a record that wraps: the overwritten slot's leaves are p_new, and the root is a full rebuild from the leaves (check())
    slot = pair.ring.pushed % T
    p_new = pair.ring.p_new
    pair.push(1)
    leaves = pair.leaves()
    assert np.all(leaves[slot] == p_new) and p_new == pair.ring.p_new
    pair.check("wrapped once more")
    pair.close()


def test_known_answer_with_equal_priorities(sim, bid):
    pair = Pair(sim, bid, 7, rng=1)
    for count in (3, 7):                                        # half filled, then full
        pair.push(count - pair.ring.count)
        n = count * N
        pushed, total, p_new = pair.reps[0].priority_state()
        assert (pushed, total, p_new) == (count, float(n), 1.0)
        got = pair.sample(4)
        w = pr.philox4x32_10(np.stack([np.arange(B), np.full(B, 4), np.full(B, 6), np.zeros(B)], axis=1).astype(np.uint32), pr._key(RSEED))
        r = ((w[:, 0] >> np.uint32(5)).astype(np.float64) * 2.0 ** 26 + (w[:, 1] >> np.uint32(6)).astype(np.float64)) * 2.0 ** -53
        leaf = np.floor(((np.arange(B) + r) / B) * n).astype(np.int64)
        assert np.array_equal(got["index"][:, 1].astype(np.int64) * N + got["index"][:, 0], leaf)
        assert np.all(got["prob"] == np.float32(1.0 / n)) and got["index"][:, 1].max() < count
    pair.close()


def test_dynamic_range(sim, bid):
    pair = Pair(sim, bid, 7, p=(1e-30, 1e-30, 1e30), rng=2)
    pair.push(5)
    cells = np.array([[0, 0, 0, 0], [69, 4, 0, 0], [33, 2, 0, 0], [64, 2, 0, 0], [63, 1, 0, 0]], np.int32)
    pair.update(pair.ring.pushed, cells, np.full(5, 1e38, np.float32))
    leaves = pair.leaves()
    assert (leaves == np.float32(1e30)).sum() == 5 and (leaves == np.float32(1e-30)).sum() == 5 * N - 5 and not leaves[5:].any()
    pair.check("handful at p_max", draws=(0, 1, 2))
    got = pair.sample(3)
    assert np.all(leaves[got["index"][:, 1], got["index"][:, 0]] > 0) and got["index"][:, 1].max() < 5
    pair.close()


def test_windows_start_at_the_prioritised_cell(sim, bid):
    pair = Pair(sim, bid, 7, rng=3)
    pair.push(5)
    rng = np.random.default_rng(9)
    index = pair.sample(0)["index"]
    pair.update(pair.ring.pushed, index, (10.0 ** rng.uniform(-3, 2, B)).astype(np.float32))
    pair.push(4)                                                # wraps
    single = pair.sample(6)
    view = pair.ring.prioritised()
    for L in (1, 3, 7):
        got, want = pair.sample_seq(6, L), seq.sample_seq(view, 6, B, L, HER, GAMMA)
        for name in seq.SEQ_FIELDS:
            assert same(got[name], want[name]), (L, name)
        assert same(got["index"], single["index"]) and same(got["prob"], single["prob"]), L
        # inside the episode: every valid step carries the ep_id of the first, in the slots that follow it
        e, slot = got["index"][:, 0], got["index"][:, 1]
        j = (slot - (pair.ring.pushed - pair.ring.count)) % pair.T
        for k in range(L):
            valid = k < got["length"]
            assert np.all(j[valid] + k < pair.ring.count)
            s = pair.ring.slot(j[valid] + k)
            assert np.all(pair.ring.ep_id[s, e[valid]] == pair.ring.ep_id[slot[valid], e[valid]]), (L, k)
        if L > 1:
            assert (got["length"] > 1).any() and (got["length"] < L).any()
    one = pair.sample_seq(6, 1)
    for name in ("obs", "action", "next_obs", "achieved_next", "reward", "done"):
        assert same(one[name][:, 0], single[name]), name
    assert same(one["goal"], single["goal"]) and same(one["nstep_obs"], single["next_obs"]) and np.all(one["length"] == 1)
    pair.close()


def test_uniform_sampler_unchanged_on_a_replay_with_priorities(sim, bid):
    pair = Pair(sim, bid, 7, rng=4)
    pair.push(9)
    pair.update(pair.ring.pushed, pair.sample(0)["index"], np.linspace(0.01, 50, B).astype(np.float32))
    for her in (0.0, 0.5, 1.0):
        got, want = pair.sample(3, her=her, uniform=True), pair.ring.sample(3, B, her)
        for name in FIELDS:
            assert same(got[name], want[name]), (her, name)
    pair.close()


def test_refused_calls_leave_no_trace(sim, bid):
    def refused(call, name):
        with pytest.raises(AssertionError, match=name):
            call()

    plain = Pair(sim, bid, 7, enable=False, rng=5)
    plain.push(2)
    refused(lambda: plain.sample(0), "hsr_replay_priority_sample_dev")                       # sample before enable
    refused(lambda: plain.reps[0].priority_enable(PrioritySpec(1.0, 1e-6, 1e6, MAX_BATCH)), "hsr_replay_priority_enable")        # enable after a commit
    refused(lambda: plain.reps[0].priority_state(), "hsr_replay_priority_state")
    assert plain.reps[0].state() == (2, 2, 2)
    for name in FIELDS:
        assert same(plain.sample(1, uniform=True)[name], plain.ring.sample(1, B, HER)[name]), name
    plain.close()
    for bad in ((1.0, 0.0, 2.0), (1.0, 2.0, 4.0), (8.0, 2.0, 4.0), (1.0, 0.5, float("inf")), (float("nan"), 0.5, 2.0)):
        fresh = Pair(sim, bid, 7, enable=False)
        refused(lambda: fresh.reps[0].priority_enable(PrioritySpec(*bad, MAX_BATCH)), "hsr_replay_priority_enable")
        fresh.close()

    pair = Pair(sim, bid, 7, rng=6)
    refused(lambda: pair.sample(0), "hsr_replay_priority_sample_dev")                        # empty
    pair.push(4)
    index = pair.sample(0)["index"]
    pair.update(pair.ring.pushed, index, np.linspace(0.1, 9, B).astype(np.float32))
    leaves, books, state = pair.leaves(), pair.reps[0].state(), pair.reps[0].priority_state()
    refused(lambda: pair.sample(0, batch=MAX_BATCH + 1), "hsr_replay_priority_sample_dev")
    refused(lambda: pair.sample(0, batch=0), "hsr_replay_priority_sample_dev")
    refused(lambda: pair.sample(0, her=1.5), "hsr_replay_priority_sample_dev")
    refused(lambda: pair.sample_seq(0, 8), "hsr_replay_priority_sample_seq_dev")
    refused(lambda: pair.sample_seq(0, 2, batch=MAX_BATCH + 1), "hsr_replay_priority_sample_seq_dev")
    refused(lambda: pair.update(5, index, np.ones(B, np.float32), mirror=False), "hsr_replay_priority_update_dev")          # sampled_at > pushed
    refused(lambda: pair.update(4, np.zeros((MAX_BATCH + 1, 4), np.int32), np.ones(MAX_BATCH + 1, np.float32), mirror=False), "hsr_replay_priority_update_dev")
    refused(lambda: pair.reps[0].priority_enable(PrioritySpec(1.0, 1e-6, 1e6, MAX_BATCH)), "hsr_replay_priority_enable")
    assert same(pair.leaves(), leaves) and pair.reps[0].state() == books and pair.reps[0].priority_state() == state
    pair.check("after the refusals")
    pair.record()                                                                            # a pending record
    pair.sim.sync()
    leaves, books, state = pair.leaves(), pair.reps[0].state(), pair.reps[0].priority_state()
    assert np.all(leaves[4] == pair.ring.p_new) and same(leaves, pair.ring.leaves)
    refused(lambda: pair.sample(0), "hsr_replay_priority_sample_dev")
    refused(lambda: pair.sample_seq(0, 2), "hsr_replay_priority_sample_seq_dev")
    assert same(pair.leaves(), leaves) and pair.reps[0].state() == books and pair.reps[0].priority_state() == state
    pair.commit()
    pair.sim.sync()
    pair.check("after the commit")
    # clear: the tree is zero, p_new is p_init again, and priorities may not be enabled twice
    pair.reps[0].clear()
    pair.ring.clear()
    assert not pair.leaves().any() and pair.reps[0].priority_state() == (0, 0.0, 1.0)
    pair.push(2)
    pair.check("after a clear")
    pair.close()


def test_env_surface_draws_by_priority_and_weighs(models):
    m = models["cfg3"]
    env = VecHSREnv(model=m, goals=[GoalSpec("block0", GOAL, GEOFENCE)], starts={"block0joint": BLOCK_START}, steps_per_action=5, n_envs=5,
                    obs_type="openai", auto_reset=True, max_episode_steps=3)
    cap, batch, beta = 8, 64, 0.4
    replay = env.make_replay(cap, her_ratio=0.5, prioritized=True, alpha=0.6, eps=1e-6)
    env.reset()
    rng = np.random.default_rng(6)
    for _ in range(5):
        env.step(rng.uniform(-1, 1, (5, m.nu)).astype(np.float32))
    out = replay.sample(batch, beta=beta)
    env.sim.sync()
    assert set(out) == set(FIELDS) | {"prob", "weight", "sampled_at"} and out["sampled_at"] == 5
    assert np.all(out["prob"].cpu().numpy() == np.float32(1 / 25))
    assert np.all(out["weight"].cpu().numpy() == 1)
    index = out["index"].cpu().numpy().copy()
    td = torch.zeros(batch, dtype=torch.float32, device=DEV)
    td[0] = 1e4
    replay.update_priorities(out, td)
    out = replay.sample(batch, beta=beta)
    env.sim.sync()
    leaves = torch.zeros((cap, 5), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    replay._replay.priority_read_dev(leaves.data_ptr())
    env.sim.sync()
    leaves = leaves.cpu().numpy()
    e0, s0 = index[0, 0], index[0, 1]
    big, small = np.float32(np.float32(1e4 + 1e-6) ** np.float32(0.6)), np.float32(1e-6) ** np.float32(0.6)
    assert abs(leaves[s0, e0] / big - 1) < 1e-5 and np.all(leaves[5:] == 0)
    touched = np.zeros((cap, 5), bool)
    touched[index[:, 1], index[:, 0]] = True
    touched[s0, e0] = False
    rest = ~touched
    rest[5:], rest[s0, e0] = False, False
    assert np.all(np.abs(leaves[touched] / small - 1) < 1e-5) and np.all(leaves[rest] == 1)
    # the restatement, given the device's leaves: the second sample is draw 1 of the env's seed
    ring = pr.PrioRing(5, cap, 25, m.nu, GEOFENCE, seed=replay._replay.spec.seed, env_offset=replay._replay.spec.env_offset, p_min=1e-30, p_max=1e30)
    ring.commit(np.zeros((5, 25), np.float32))
    for _ in range(5):
        ring.record(*[np.zeros(s, np.float32) for s in ((5, m.nu), (5, 25), (5,), (5,), (5, 3), (5, 3))])
        ring.commit(np.zeros((5, 25), np.float32))
    ring.leaves = leaves
    e, j, *_, prob = ring.prio_indices(1, batch, 0.5)
    got = out["index"].cpu().numpy()
    assert np.array_equal(got[:, 0], e) and np.array_equal(got[:, 1], ring.slot(j)) and same(out["prob"].cpu().numpy(), prob)
    hits = int(((got[:, 0] == e0) & (got[:, 1] == s0)).sum())
    assert hits == int(((e == e0) & (ring.slot(j) == s0)).sum()) and hits > batch // 2
    # weight = (n prob)^-beta over its maximum: the torch expression rounds n prob, the power (a few ulp), the maximum's power and the
    # quotient to float32 - 8 ulp (2^-23 each) cover that
    w, p64 = out["weight"].cpu().numpy(), out["prob"].cpu().numpy().astype(np.float64)
    want = (25 * p64) ** -beta
    want = want / want.max()
    assert w.max() == 1 and np.all(np.abs(w / want - 1) <= 8 * 2.0 ** -23), np.abs(w / want - 1).max()
    env.close()
