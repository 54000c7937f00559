"""The numpy restatement of the window sampler (tests/replay_seq_ref.py) has the properties its specification states (include/hsrsim.h:
hsr_replay_sample_seq_dev) before tests/test_gpu_replay_seq.py holds the device to it.  No GPU.

Synthetic rings of the GPU test's main shape: 70 envs, a ring of 7 steps that wraps, 12 steps, episodes that end with a success or after
`limit` steps, achieved and desired points spread so that roughly a third of the steps succeed."""
from fractions import Fraction

import numpy as np
import pytest

import replay_ref as ref
import replay_seq_ref as seq


def synthetic(n_envs=70, capacity=7, steps=12, limit=3, seed=3, geofence=0.05, ring_seed=11):
    rng = np.random.default_rng(seed)
    od, nu = 5, 2
    ring = ref.Ring(n_envs, capacity, od, nu, geofence, seed=ring_seed)
    ring.commit(rng.normal(size=(n_envs, od)))
    ep_step = np.zeros(n_envs, np.int64)
    for _ in range(steps):
        ach, des = rng.uniform(-0.05, 0.05, (n_envs, 3)), rng.uniform(-0.05, 0.05, (n_envs, 3))
        done = ref.within(ach, des, geofence)
        ring.record(rng.normal(size=(n_envs, nu)), rng.normal(size=(n_envs, od)), done.astype(np.float32), done, ach, des)
        ep_step += 1
        reset = done | (ep_step >= limit)
        ep_step[reset] = 0
        ring.commit(rng.normal(size=(n_envs, od)), reset)
    return ring


@pytest.fixture(scope="module")
def ring():
    return synthetic()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)


@pytest.mark.parametrize("her", [0.0, 0.5, 1.0])
def test_seq_len_one_is_the_single_step_sampler(ring, her):
    one, want = seq.sample_seq(ring, 4, 193, 1, her, 0.9), ring.sample(4, 193, her)
    for name in ("obs", "action", "next_obs", "achieved_next", "reward", "done"):
        assert same(one[name][:, 0], want[name]), name
    assert same(one["goal"], want["goal"]) and same(one["index"], want["index"])
    assert np.all(one["length"] == 1) and np.all(one["nstep"] == 1)
    assert same(one["nstep_return"], want["reward"]) and np.all(one["nstep_discount"] == np.float32(0.9))
    assert same(one["nstep_obs"], want["next_obs"]) and same(one["nstep_done"], want["done"])


@pytest.mark.parametrize("L", [2, 3, 5, 7])
def test_windows_stay_in_their_episode_and_length_is_the_slow_count(ring, L):
    out = seq.sample_seq(ring, 1, 512, L, 0.5, 0.9)
    e, j, _, _, _ = ring.indices(1, 512, 0.5)
    for i in range(512):
        # the slow way: walk forward from age j while the episode id stays and the ring has steps
        ids = [int(ring.ep_id[ring.slot(a), e[i]]) for a in range(ring.count)]
        n = 1
        while n < L and j[i] + n < ring.count and ids[j[i] + n] == ids[j[i]]:
            n += 1
        assert out["length"][i] == n, i
        for k in range(L):
            if k < n:
                s = ring.slot(j[i] + k)
                assert ring.ep_id[s, e[i]] == ids[j[i]] and ring.ep_step[s, e[i]] == ring.ep_step[ring.slot(j[i]), e[i]] + k
                assert same(out["obs"][i, k], ring.obs[s, e[i]]) and same(out["next_obs"][i, k], ring.next_obs[s, e[i]])
                assert same(out["action"][i, k], ring.act[s, e[i]]) and same(out["achieved_next"][i, k], ring.achieved[s, e[i]])
            else:
                for name in seq.PER_STEP:
                    assert not out[name][i, k].view(np.uint32 if out[name].dtype == np.float32 else np.uint8).any(), (name, i, k)
    assert (out["length"] < L).any() and (out["length"] > 1).any()
    assert 1 <= out["length"].min() and out["length"].max() <= min(L, 3)


def test_nstep_against_exact_arithmetic(ring):
    """Rewards 0 / 1 and gamma 0.5: every partial sum is a dyadic rational of a few bits, so float32 is exact and a Fraction says what it is."""
    for her in (0.0, 1.0):
        out = seq.sample_seq(ring, 2, 1024, 3, her, 0.5)
        assert set(np.unique(out["reward"]).tolist()) <= {0.0, 1.0}
        for i in range(1024):
            n, r, d = int(out["length"][i]), out["reward"][i], out["done"][i]
            m = next((k + 1 for k in range(n) if d[k]), n)
            acc = sum(Fraction(1, 2 ** k) * int(r[k]) for k in range(m))
            assert out["nstep"][i] == m and Fraction(float(out["nstep_return"][i])) == acc and Fraction(float(out["nstep_discount"][i])) == Fraction(1, 2 ** m)
            assert out["nstep_done"][i] == d[m - 1]
            e, sj = out["index"][i, :2]
            age = (sj - ring.slot(0)) % ring.T
            assert same(out["nstep_obs"][i], ring.next_obs[ring.slot(age + m - 1), e])
        assert (out["nstep"] > 1).any()
    # the chain as a function of its own: done first, in the middle, never; one step; gamma 0 and 1
    f = lambda r, d, n, g: seq.nstep(np.array(r, np.float32), np.array(d, np.uint8), n, g)
    assert f([1, 1, 1], [1, 0, 0], 3, 0.5) == (1, 1.0, 0.5, 1)
    assert f([0, 1, 1], [0, 1, 0], 3, 0.5) == (2, 0.5, 0.25, 1)
    assert f([1, 1, 1], [0, 0, 0], 3, 0.5) == (3, 1.75, 0.125, 0)
    assert f([1, 1, 1], [0, 0, 1], 2, 0.5) == (2, 1.5, 0.25, 0)                # the window ends before the done step
    assert f([3], [0], 1, 0.9) == (1, 3.0, np.float32(0.9), 0)
    assert f([1, 1, 1], [0, 0, 0], 3, 0.0) == (3, 1.0, 0.0, 0) and f([1, 1, 1], [0, 0, 0], 3, 1.0) == (3, 3.0, 1.0, 0)


def test_a_relabelled_window_that_covers_its_episode_ends_done(ring):
    """her_ratio = 1, seq_len >= the episode limit: the goal is the achieved point of a step of the window, that step reaches it
    (distance 0), so the chain stops at or before it with nstep_done = 1 - for every sample."""
    out = seq.sample_seq(ring, 9, 4096, 3, 1.0, 0.9)
    _, j, relabel, j_end, j_goal = ring.indices(9, 4096, 1.0)
    assert relabel.all()
    assert np.all(j_goal - j < out["length"])                                    # the goal step lies inside the window
    assert np.all(out["nstep"] <= j_goal - j + 1)
    exceptions = int((out["nstep_done"] != 1).sum())
    print(f"{exceptions} of 4096 windows do not end with nstep_done = 1")
    assert exceptions == 0
    assert np.all(out["reward"][np.arange(4096), out["nstep"] - 1] == 1)
    # the cases the GPU test asks its own restatement for occur on this ring too
    counts = [int(((1 < out["nstep"]) & (out["nstep"] < out["length"])).sum()), int(((out["nstep"] == out["length"]) & (out["length"] > 1)).sum()),
              int((out["length"] < 3).sum()), int((seq.sample_seq(ring, 9, 4096, 3, 0.0, 0.9)["nstep_done"] == 0).sum())]
    print(f"1 < nstep < length: {counts[0]}, nstep == length > 1: {counts[1]}, length < seq_len: {counts[2]}, her 0 and not done: {counts[3]}")
    assert min(counts) >= 10


def test_arguments_are_refused(ring):
    for bad in (dict(seq_len=0), dict(seq_len=8), dict(gamma=np.nan), dict(gamma=-0.1), dict(gamma=1.5), dict(batch=0), dict(her_ratio=1.5)):
        kw = {**dict(draw=0, batch=4, seq_len=2, her_ratio=0.5, gamma=0.9), **bad}
        with pytest.raises(ref.OutOfOrder):
            seq.sample_seq(ring, **kw)
    assert seq.sample_seq(ring, 0, 4, 7, 0.5, 1.0)["obs"].shape == (4, 7, 5)
