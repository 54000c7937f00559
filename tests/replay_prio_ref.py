"""Checker-side restatement of the device replay's priorities (include/hsrsim.h: hsr_replay_priority_*), in numpy, written from that
specification on top of replay_ref.Ring and not from the kernels: the float64 binary sum tree over the float32 leaves, the descent rule,
the stratified draw, the update with its clamp, duplicate and staleness rules, and p_new.  The product never imports it.

The tree is the plain binary one: 2^h >= T N leaves, absent leaves 0, every inner node left + right in float64.  Every float64 operation
of the draw is a numpy float64 operation of its own; leaves are float32 and only ever stored, compared and widened."""
import numpy as np

from episode_ref import MASK, _key, philox4x32_10
from replay_ref import EMPTY, PENDING, OutOfOrder, Ring, mulhi

STREAM_PRIO = 6


def build_tree(leaves):
    """[level 0 = the leaves padded to 2^h as float64, level 1, .., the root (one value)]."""
    flat = np.asarray(leaves, np.float32).reshape(-1)
    h = max(int(np.ceil(np.log2(flat.size))), 0)
    while (1 << h) < flat.size:
        h += 1
    level = np.zeros(1 << h, np.float64)
    level[:flat.size] = flat.astype(np.float64)
    levels = [level]
    while level.size > 1:
        level = level[0::2] + level[1::2]
        levels.append(level)
    return levels


def descend(levels, u):
    """The leaf every target u (float64 [B]) reaches: left if u < l or r == 0, else u -= l and right."""
    u = np.array(u, np.float64)
    at = np.zeros(u.shape, np.int64)
    for level in levels[-2::-1]:
        l, r = level[2 * at], level[2 * at + 1]
        left = (u < l) | (r == 0)
        u = np.where(left, u, u - l)
        at = 2 * at + (~left).astype(np.int64)
    return at


def clamp(x, p_min, p_max):
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), np.float32(p_max), np.minimum(np.maximum(x, np.float32(p_min)), np.float32(p_max))).astype(np.float32)


def newest_record_of_slot(written, T, slot):
    """k_s: the largest k < written with k mod T == slot, or None."""
    ks = [k for k in range(written) if k % T == slot]
    return ks[-1] if ks else None


class PrioRing(Ring):
    def __init__(self, n_envs, capacity_steps, obs_dim, nu, geofence, seed=0, env_offset=0, p_init=1.0, p_min=1e-6, p_max=1e6, max_batch=4096):
        self.p_init, self.p_min, self.p_max, self.max_batch = np.float32(p_init), np.float32(p_min), np.float32(p_max), int(max_batch)
        assert np.isfinite([self.p_init, self.p_min, self.p_max]).all() and 0 < self.p_min <= self.p_init <= self.p_max
        assert int(n_envs) * int(capacity_steps) <= 2 ** 30
        super().__init__(n_envs, capacity_steps, obs_dim, nu, geofence, seed=seed, env_offset=env_offset)

    # ---- protocol
    def clear(self):
        super().clear()
        self.leaves = np.zeros((self.T, self.N), np.float32)
        self.p_new = self.p_init

    def record(self, *args):
        slot = self.pushed % self.T
        super().record(*args)
        self.leaves[slot] = self.p_new

    @property
    def total(self):
        return float(build_tree(self.leaves)[-1][0])

    # ---- the draw
    def prio_indices(self, draw, batch, her_ratio):
        """(env, age, relabelled, last age of the episode, goal age, prob) of every sample."""
        her = np.float32(her_ratio)
        if self.state == PENDING or self.count == 0 or batch < 1 or batch > self.max_batch or not np.isfinite(her) or her < 0 or her > 1:
            raise OutOfOrder("prioritised sample")
        ctr = np.zeros((batch, 4), np.uint32)
        ctr[:, 0] = np.arange(batch, dtype=np.uint32); ctr[:, 1] = np.uint32(int(draw) & MASK); ctr[:, 2] = STREAM_PRIO; ctr[:, 3] = np.uint32(self.env_offset)
        w = philox4x32_10(ctr, _key(self.seed))
        levels = build_tree(self.leaves)
        total = levels[-1][0]
        frac = ((w[:, 0] >> np.uint32(5)).astype(np.uint64) * np.uint64(1 << 26) + (w[:, 1] >> np.uint32(6)).astype(np.uint64)).astype(np.float64) * np.float64(2.0 ** -53)
        u = (np.arange(batch, dtype=np.float64) + frac) / np.float64(batch)
        u = u * total
        leaf = descend(levels, u)
        assert leaf.max() < self.T * self.N
        slot, e = leaf // self.N, leaf % self.N
        first = (self.pushed - self.count) % self.T
        j = (slot - first + self.T) % self.T
        prob = (self.leaves[slot, e].astype(np.float64) / total).astype(np.float32)
        relabel = (w[:, 2] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24) < her
        ages = np.arange(self.count, dtype=np.int64)
        ids = self.ep_id[self.slot(ages)[:, None], e[None, :]]
        differs = (ages[:, None] > j[None, :]) & (ids != ids[np.minimum(j, self.count - 1), np.arange(batch)][None, :])
        j_end = np.where(differs.any(0), differs.argmax(0), self.count) - 1
        j_goal = j + mulhi(w[:, 3], j_end - j + 1)
        return e, j, relabel, j_end, j_goal, prob

    def prioritised(self):
        """The ring as the prioritised samplers see it: Ring.sample and replay_seq_ref.sample_seq applied to it take the prioritised draw."""
        return Prioritised(self)

    def prio_sample(self, draw, batch, her_ratio):
        out = self.prioritised().sample(draw, batch, her_ratio)
        out["prob"] = self.prio_indices(draw, batch, her_ratio)[5]
        return out

    # ---- update
    def update(self, sampled_at, index, priority):
        index, priority = np.asarray(index, np.int64), np.asarray(priority, np.float32)
        batch = len(priority)
        if self.count == 0 or batch < 1 or batch > self.max_batch or sampled_at > self.pushed:
            raise OutOfOrder("update")
        written = self.pushed + (1 if self.state == PENDING else 0)
        stored = {}
        for (e, slot), x in zip(index[:, :2], clamp(priority, self.p_min, self.p_max)):
            if not (0 <= e < self.N and 0 <= slot < self.T):
                continue
            k_s = newest_record_of_slot(written, self.T, int(slot))
            if k_s is None or not k_s < sampled_at:
                continue
            cell = (int(slot), int(e))
            stored[cell] = max(stored.get(cell, np.float32(0)), x)
        for cell, x in stored.items():
            self.leaves[cell] = x
            self.p_new = max(self.p_new, x)


class Prioritised:
    def __init__(self, ring):
        self._ring = ring

    def __getattr__(self, name):
        return getattr(self._ring, name)

    def indices(self, draw, batch, her_ratio):
        return self._ring.prio_indices(draw, batch, her_ratio)[:5]

    def sample(self, draw, batch, her_ratio):
        return Ring.sample(self, draw, batch, her_ratio)
