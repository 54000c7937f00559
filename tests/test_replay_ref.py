"""The numpy restatement of the hindsight replay (tests/replay_ref.py) has the properties its specification states (include/hsrsim.h:
hsr_replay_sample_dev) before tests/test_gpu_replay.py holds the device to it.  No GPU."""
import numpy as np
import pytest

import replay_ref as ref


def filled(n_envs, capacity, steps, seed=3, p_reset=0.3, spread=0.05, geofence=0.05, ring_seed=11):
    """A ring after `steps` transitions of random rows; an env starts a new episode after a step with probability p_reset."""
    rng = np.random.default_rng(seed)
    od, nu = 5, 2
    ring = ref.Ring(n_envs, capacity, od, nu, geofence, seed=ring_seed)
    ring.commit(rng.normal(size=(n_envs, od)))
    for _ in range(steps):
        ach = rng.uniform(-spread, spread, (n_envs, 3))
        des = rng.uniform(-spread, spread, (n_envs, 3))
        done = ref.within(ach, des, geofence)
        ring.record(rng.normal(size=(n_envs, nu)), rng.normal(size=(n_envs, od)), done.astype(np.float32), done, ach, des)
        ring.commit(rng.normal(size=(n_envs, od)), rng.random(n_envs) < p_reset)
    return ring


@pytest.mark.parametrize("pushed", [3, 7, 12])
def test_ages_and_slots_wrap(pushed):
    """T = 7: fewer steps than the ring holds, exactly as many, and more - age 0 is the oldest kept step, the newest sits before the head."""
    T = 7
    ring = filled(4, T, pushed)
    count = min(pushed, T)
    assert ring.pushed == pushed and ring.count == count and ring.head_slot == pushed % T
    steps = np.arange(pushed - count, pushed)                  # the env-steps still kept, oldest first
    assert np.array_equal(ring.slot(np.arange(count)), steps % T)
    assert ring.slot(count - 1) == (pushed - 1) % T
    # per env, ids never decrease with age, and a step counter restarts exactly where the id changes
    ids, st = ring.ep_id[ring.slot(np.arange(count))].astype(np.int64), ring.ep_step[ring.slot(np.arange(count))].astype(np.int64)
    assert np.all(np.diff(ids, axis=0) >= 0)
    assert np.array_equal(np.diff(ids, axis=0) > 0, st[1:] == 0) and np.all(st[1:][np.diff(ids, axis=0) == 0] == st[:-1][np.diff(ids, axis=0) == 0] + 1)


def test_protocol_refuses_calls_out_of_order():
    ring = ref.Ring(2, 3, 4, 1, 0.05)
    z = lambda *s: np.zeros(s, np.float32)
    with pytest.raises(ref.OutOfOrder):
        ring.record(z(2, 1), z(2, 4), z(2), z(2), z(2, 3), z(2, 3))
    with pytest.raises(ref.OutOfOrder):
        ring.sample(0, 4, 0.5)                                 # empty
    ring.commit(z(2, 4))
    ring.record(z(2, 1), z(2, 4), z(2), z(2), z(2, 3), z(2, 3))
    with pytest.raises(ref.OutOfOrder):
        ring.record(z(2, 1), z(2, 4), z(2), z(2), z(2, 3), z(2, 3))
    with pytest.raises(ref.OutOfOrder):
        ring.sample(0, 4, 0.5)                                 # pending
    ring.commit(z(2, 4), np.zeros(2))
    assert ring.pushed == 1 and ring.sample(0, 4, 0.5)["obs"].shape == (4, 4)
    for bad in (-0.1, 1.5, np.nan, np.inf):
        with pytest.raises(ref.OutOfOrder):
            ring.sample(0, 4, bad)
    with pytest.raises(ref.OutOfOrder):
        ring.sample(0, 0, 0.5)
    ring.clear()
    assert ring.pushed == 0 and ring.state == ref.EMPTY and not ring.cur_id.any()


def test_goal_age_stays_in_the_episode_and_not_before_the_step():
    ring = filled(9, 7, 12)
    for draw in range(4):
        e, j, relabel, j_end, j_goal = ring.indices(draw, 2048, 1.0)
        assert relabel.all() and np.all((0 <= j) & (j <= j_goal) & (j_goal <= j_end) & (j_end < ring.count))
        ids = lambda a: ring.ep_id[ring.slot(a), e]
        assert np.array_equal(ids(j), ids(j_goal)) and np.array_equal(ids(j), ids(j_end))
        last = j_end == ring.count - 1
        assert np.all(ids(np.minimum(j_end + 1, ring.count - 1))[~last] != ids(j)[~last])      # j_end is the LAST age of the episode
        assert np.all(ring.ep_step[ring.slot(j_goal), e] >= ring.ep_step[ring.slot(j), e])
    # the uniform draw over the rest of the episode reaches its end and its start
    assert (j_goal == j_end).any() and (j_goal == j).any() and (j_goal > j).any()


def test_her_ratio_zero_never_relabels_and_one_always_does():
    ring = filled(5, 6, 9)
    never, always = ring.sample(1, 4096, 0.0), ring.sample(1, 4096, 1.0)
    assert not never["index"][:, 3].any() and np.all(never["index"][:, 2] == -1)
    assert always["index"][:, 3].all() and np.all(always["index"][:, 2] >= 0)
    e, s = never["index"][:, 0], never["index"][:, 1]
    assert np.array_equal(never["goal"], ring.desired[s, e]) and np.array_equal(never["reward"], ring.reward[s, e])
    assert np.array_equal(never["done"], ring.done[s, e])
    assert np.array_equal(always["index"][:, :2], never["index"][:, :2])        # the relabel draw does not move the transition draw


def test_relabelled_share_is_the_ratio():
    """B = 4096 Bernoulli(0.8) draws: the share lies within four standard deviations, 4 sqrt(0.8 0.2 / 4096) = 0.025 (the run is
    deterministic for the seed)."""
    ring = filled(5, 6, 9)
    share = ring.sample(0, 4096, 0.8)["index"][:, 3].mean()
    assert abs(share - 0.8) <= 0.025, share


def test_every_env_and_age_is_drawn():
    ring = filled(5, 6, 9)
    idx = ring.sample(2, 4096, 0.8)["index"]
    assert len({(int(e), int(s)) for e, s in idx[:, :2]}) == 5 * 6


def test_a_goal_taken_from_the_step_itself_gives_reward_one():
    ring = filled(5, 6, 9)
    out = ring.sample(3, 4096, 1.0)
    own = out["index"][:, 2] == out["index"][:, 1]
    assert own.sum() > 100 and np.all(out["reward"][own] == 1) and np.all(out["done"][own] == 1)
    assert np.array_equal(out["goal"][own], out["achieved_next"][own])
    assert (out["reward"] == 0).any()                          # and a goal from a later step does not always hold
    assert np.array_equal(out["done"], (out["reward"] != 0).astype(np.uint8))


def test_another_draw_or_shard_gives_other_samples():
    a = filled(5, 6, 9)
    b = filled(5, 6, 9)
    b.env_offset = 70
    same = lambda x, y: np.array_equal(x["index"], y["index"])
    assert same(a.sample(0, 256, 0.5), a.sample(0, 256, 0.5)) and not same(a.sample(0, 256, 0.5), a.sample(1, 256, 0.5))
    assert not same(a.sample(0, 256, 0.5), b.sample(0, 256, 0.5))


def test_row_words():
    assert ref.row_words(17, 2) == (46, 48) and ref.row_words(27, 7) == (71, 72) and ref.row_words(25, 7) == (67, 68)
