"""Checker-side restatement of the device hindsight replay, in numpy, written from its specification (include/hsrsim.h: hsr_replay_spec ..
hsr_replay_sample_dev) and not from the kernels: the ring and its protocol, the replay's own episode counters, the index draw and the
relabel.  The product never imports it.

Rows are kept as float32 / uint32 arrays and only ever copied, so bit patterns survive as they do on the device.  The one float
computation is the relabelled reward: norm(achieved - goal) < geofence with the difference, the three squares, the two sums and the
square root each a float32 operation of its own.  (The device may contract a product and a sum into one fma; the distances then differ in
the last bit, which changes the compare only for a distance within an ulp of the geofence.)
"""
import numpy as np

from episode_ref import MASK, _key, philox4x32_10

STREAM_REPLAY = 4
EMPTY, READY, PENDING = 0, 1, 2


class OutOfOrder(Exception):
    """A call the protocol refuses (the device returns HSR_EINVAL and launches nothing)."""


def row_words(obs_dim, nu):
    """(W, W padded to a multiple of 4)."""
    w = 2 * obs_dim + nu + 10
    return w, (w + 3) // 4 * 4


def mulhi(words, n):
    return ((np.asarray(words, np.uint32).astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def within(a, g, geofence):
    """norm(a - g) < geofence in float32, operation by operation."""
    d = (np.asarray(a, np.float32) - np.asarray(g, np.float32)).astype(np.float32)
    sq = (d * d).astype(np.float32)
    s = ((sq[..., 0] + sq[..., 1]).astype(np.float32) + sq[..., 2]).astype(np.float32)
    return np.sqrt(s).astype(np.float32) < np.float32(geofence)


class Ring:
    def __init__(self, n_envs, capacity_steps, obs_dim, nu, geofence, seed=0, env_offset=0):
        self.N, self.T, self.obs_dim, self.nu = int(n_envs), int(capacity_steps), int(obs_dim), int(nu)
        self.geofence, self.seed, self.env_offset = np.float32(geofence), int(seed), int(env_offset) & MASK
        T, N = self.T, self.N
        f32 = lambda *s: np.zeros(s, np.float32)
        self.obs, self.act, self.next_obs = f32(T, N, obs_dim), f32(T, N, nu), f32(T, N, obs_dim)
        self.achieved, self.desired, self.reward = f32(T, N, 3), f32(T, N, 3), f32(T, N)
        self.done, self.ep_id, self.ep_step = np.zeros((T, N), np.uint8), np.zeros((T, N), np.uint32), np.zeros((T, N), np.uint32)
        self.head = f32(N, obs_dim)
        self.clear()

    # ---- protocol
    def clear(self):
        self.state, self.pushed = EMPTY, 0
        self.cur_id, self.cur_step = np.zeros(self.N, np.uint32), np.zeros(self.N, np.uint32)

    def commit(self, obs, reset=None):
        self.head = np.array(obs, np.float32).reshape(self.N, self.obs_dim)
        on = np.ones(self.N, bool) if reset is None else np.asarray(reset).reshape(self.N) != 0
        self.cur_id = np.where(on, self.cur_id + np.uint32(1), self.cur_id).astype(np.uint32)
        self.cur_step = np.where(on, np.uint32(0), self.cur_step + np.uint32(1)).astype(np.uint32)
        if self.state == PENDING:
            self.pushed += 1
        self.state = READY

    def record(self, ctrl, next_obs, reward, done, achieved, desired):
        if self.state != READY:
            raise OutOfOrder("record before commit" if self.state == EMPTY else "two records")
        s = self.pushed % self.T
        self.obs[s], self.act[s], self.next_obs[s] = self.head, np.asarray(ctrl, np.float32), np.asarray(next_obs, np.float32)
        self.reward[s], self.done[s] = np.asarray(reward, np.float32), (np.asarray(done) != 0).astype(np.uint8)
        self.achieved[s], self.desired[s] = np.asarray(achieved, np.float32), np.asarray(desired, np.float32)
        self.ep_id[s], self.ep_step[s] = self.cur_id, self.cur_step
        self.state = PENDING

    # ---- books
    @property
    def count(self):
        return min(self.pushed, self.T)

    @property
    def head_slot(self):
        return self.pushed % self.T

    def slot(self, age):
        return (self.pushed - self.count + np.asarray(age, np.int64)) % self.T

    # ---- sampling
    def indices(self, draw, batch, her_ratio):
        """(env, age, relabelled, last age of the episode, goal age) of every sample: int64 / bool arrays [batch]."""
        her = np.float32(her_ratio)
        if self.state == PENDING or self.count == 0 or batch < 1 or not np.isfinite(her) or her < 0 or her > 1:
            raise OutOfOrder("sample")
        ctr = np.zeros((batch, 4), np.uint32)
        ctr[:, 0] = np.arange(batch, dtype=np.uint32); ctr[:, 1] = np.uint32(int(draw) & MASK); ctr[:, 2] = STREAM_REPLAY; ctr[:, 3] = np.uint32(self.env_offset)
        w = philox4x32_10(ctr, _key(self.seed))
        e, j = mulhi(w[:, 0], self.N), mulhi(w[:, 1], self.count)
        u = (w[:, 2] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
        relabel = u < her
        ages = np.arange(self.count, dtype=np.int64)
        ids = self.ep_id[self.slot(ages)[:, None], e[None, :]]                  # [count, batch]: the env's ids, oldest first
        differs = (ages[:, None] > j[None, :]) & (ids != ids[j, np.arange(batch)][None, :])
        j_end = np.where(differs.any(0), differs.argmax(0), self.count) - 1
        j_goal = j + mulhi(w[:, 3], j_end - j + 1)
        return e, j, relabel, j_end, j_goal

    def sample(self, draw, batch, her_ratio):
        e, j, relabel, _, j_goal = self.indices(draw, batch, her_ratio)
        s, sg = self.slot(j), self.slot(j_goal)
        achieved = self.achieved[s, e]
        goal = np.where(relabel[:, None], self.achieved[sg, e], self.desired[s, e]).astype(np.float32)
        # np.where copies bit patterns; the reward of a relabelled sample is the goal test on the new goal
        reach = within(achieved, goal, self.geofence)
        reward = np.where(relabel, reach.astype(np.float32), self.reward[s, e]).astype(np.float32)
        done = np.where(relabel, reach, self.done[s, e] != 0).astype(np.uint8)
        index = np.stack([e, s, np.where(relabel, sg, -1), relabel.astype(np.int64)], axis=1).astype(np.int32)
        return dict(obs=self.obs[s, e], action=self.act[s, e], next_obs=self.next_obs[s, e], goal=goal, achieved_next=achieved, reward=reward,
                    done=done, index=index)
