"""Checker-side restatement of the device's on-policy rollout, in numpy, written from its specification (include/hsrsim.h: hsr_rollout_spec ..
hsr_rollout_planes_dev) and not from the kernels: the store and its protocol, GAE, the statistics, the shuffle.  The product never imports it.

Rows are kept as float32 arrays and only ever copied, so bit patterns survive as they do on the device.  GAE is np.float32 operations in
the stated order, one rounding each; the statistics are fp64; Philox is episode_ref's.
"""
import numpy as np

from episode_ref import MASK, _key, philox4x32_10

STREAM_ROLLOUT = 5
EMPTY, READY, STAGED, DONE = 0, 1, 2, 3


class OutOfOrder(Exception):
    """A call the protocol refuses (the device returns HSR_EINVAL and launches nothing)."""


def row_words(obs_dim, nu):
    """(W, W padded to a multiple of 4)."""
    w = obs_dim + nu
    return w, (w + 3) // 4 * 4


def gae(reward, value, kind, v_term, last_value, gamma, lam):
    """(adv, ret) float32 [T, N] of float32 [T, N] planes (kind: integers), float32 [N] last_value.  Every operation one float32 operation."""
    reward, value, v_term = (np.asarray(x, np.float32) for x in (reward, value, v_term))
    kind, last_value = np.asarray(kind), np.asarray(last_value, np.float32)
    T, N = reward.shape
    g = np.float32(gamma)
    gl = np.float32(g * np.float32(lam))
    zero = np.zeros(N, np.float32)
    adv, ret = np.zeros((T, N), np.float32), np.zeros((T, N), np.float32)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            on = kind[t] == 0
            nv = np.where(on, last_value if t == T - 1 else value[t + 1], np.where(kind[t] == 2, v_term[t], zero)).astype(np.float32)
            delta = ((reward[t] + (g * nv).astype(np.float32)).astype(np.float32) - value[t]).astype(np.float32)
            carry = np.where(on, adv[t + 1], zero).astype(np.float32) if t < T - 1 else zero
            adv[t] = (delta + (gl * carry).astype(np.float32)).astype(np.float32)
            ret[t] = (adv[t] + value[t]).astype(np.float32)
    return adv, ret


def stats(adv):
    """(mean, std, rstd) in fp64 over all advantages, two passes."""
    a = np.asarray(adv, np.float32).astype(np.float64).reshape(-1)
    mean = a.sum() / a.size
    var = ((a - mean) ** 2).sum() / a.size
    std = np.sqrt(var)
    return mean, std, 1.0 / (std + 1e-8)


def normalized(adv, mean32, rstd32):
    """mul(sub(adv, mean32), rstd32) in float32."""
    with np.errstate(all="ignore"):
        return ((np.asarray(adv, np.float32) - np.float32(mean32)).astype(np.float32) * np.float32(rstd32)).astype(np.float32)


def round_keys(seed, epoch, env_offset):
    ctr = np.array([[int(epoch) & MASK, 0, STREAM_ROLLOUT, int(env_offset) & MASK]], np.uint32)
    return [int(w) for w in philox4x32_10(ctr, _key(seed))[0]]


def half_bits(items):
    bits = int(items - 1).bit_length()
    return max(1, (bits + 1) // 2)


def _f(v, k, mask):
    v = (v ^ np.uint64(k)) & np.uint64(MASK)
    v = (v * np.uint64(0x9E3779B1)) & np.uint64(MASK)
    v ^= v >> np.uint64(15)
    v = (v * np.uint64(0x85EBCA77)) & np.uint64(MASK)
    v ^= v >> np.uint64(13)
    return v & np.uint64(mask)


def perm(i, items, seed, epoch, env_offset):
    """perm(i) for an array of positions i < items: int64 array.  uint32 arithmetic carried in uint64 and masked."""
    keys, h = round_keys(seed, epoch, env_offset), half_bits(items)
    mask = (1 << h) - 1
    x = np.array(i, np.uint64).reshape(-1)
    assert np.all(x < items)
    todo = np.ones(x.shape, bool)
    while todo.any():
        l, r = x[todo] >> np.uint64(h), x[todo] & np.uint64(mask)
        for k in keys:
            l, r = r, l ^ _f(r, k, mask)
        x[todo] = (l << np.uint64(h)) | r
        todo = x >= items
    return x.astype(np.int64)


class Store:
    def __init__(self, n_envs, horizon, obs_dim, nu, gamma, lam, seed=0, env_offset=0):
        self.N, self.T, self.obs_dim, self.nu = int(n_envs), int(horizon), int(obs_dim), int(nu)
        self.gamma, self.lam, self.seed, self.env_offset = np.float32(gamma), np.float32(lam), int(seed), int(env_offset) & MASK
        T, N = self.T, self.N
        f32 = lambda *s: np.zeros(s, np.float32)
        self.obs, self.act = f32(T, N, obs_dim), f32(T, N, nu)
        self.logp, self.value, self.reward, self.v_term, self.adv, self.ret = (f32(T, N) for _ in range(6))
        self.kind = np.zeros((T, N), np.uint8)
        self.head = f32(N, obs_dim)
        self.state, self.t = EMPTY, 0
        self.mean32 = self.std32 = self.rstd32 = np.float32(0)

    # ---- protocol
    def begin(self, obs):
        self.head = np.array(obs, np.float32).reshape(self.N, self.obs_dim)
        self.state, self.t = READY, 0

    def stage(self, act, logp, value):
        if self.state != READY or self.t >= self.T:
            raise OutOfOrder("stage")
        t = self.t
        self.obs[t], self.act[t] = self.head, np.asarray(act, np.float32)
        self.logp[t], self.value[t] = np.asarray(logp, np.float32), np.asarray(value, np.float32)
        self.state = STAGED

    def close(self, reward, kind, next_obs):
        if self.state != STAGED:
            raise OutOfOrder("close")
        t = self.t
        self.reward[t], self.kind[t], self.v_term[t] = np.asarray(reward, np.float32), np.asarray(kind, np.uint8), 0
        self.head = np.array(next_obs, np.float32).reshape(self.N, self.obs_dim)
        self.state, self.t = READY, t + 1

    def bootstrap(self, value_terminal):
        if self.state != READY or self.t < 1:
            raise OutOfOrder("bootstrap")
        self.v_term[self.t - 1] = np.asarray(value_terminal, np.float32)

    def finish(self, last_value):
        if self.state != READY or self.t < self.T:
            raise OutOfOrder("finish")
        self.adv, self.ret = gae(self.reward, self.value, self.kind, self.v_term, last_value, self.gamma, self.lam)
        with np.errstate(all="ignore"):
            self.stats64 = stats(self.adv)
        self.mean32, self.std32, self.rstd32 = (np.float32(x) for x in self.stats64)
        self.state = DONE

    def next(self):
        if self.state != DONE:
            raise OutOfOrder("next")
        self.state, self.t = READY, 0

    # ---- minibatches
    def minibatch(self, epoch, first, count, normalize, mean32=None, rstd32=None):
        """The fields of rows first .. first + count - 1 of epoch's shuffle; the normalisation uses the given float32 mean / rstd (the
        device's own), or the restatement's."""
        items = self.T * self.N
        if self.state != DONE or count < 1 or first < 0 or first + count > items:
            raise OutOfOrder("minibatch")
        p = perm(np.arange(first, first + count), items, self.seed, epoch, self.env_offset)
        t, e = p // self.N, p % self.N
        adv = self.adv[t, e]
        if normalize:
            adv = normalized(adv, self.mean32 if mean32 is None else mean32, self.rstd32 if rstd32 is None else rstd32)
        return dict(obs=self.obs[t, e], action=self.act[t, e], logp=self.logp[t, e], value=self.value[t, e], advantage=adv, ret=self.ret[t, e],
                    index=np.stack([t, e], axis=1).astype(np.int32))
