"""Checker-side restatement of the device episode layer, in numpy, written from its specification (include/hsrsim.h: hsr_episode_spec)
and not from the kernels: Philox4x32-10, the draw layout, and the books an episode end keeps.  The product never imports it.

Every float operation is a float32 numpy operation of its own, so the draws are bit-exact against the device, which rounds every step
to float32 too; only the block quaternion goes through cos / sin and is compared with a tolerance by its test.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
STREAM_QPOS, STREAM_GOAL, STREAM_BLOCK, STREAM_CTRL = 0, 1, 2, 3


def philox4x32_10(ctr, key):
    """ctr: uint32 [..., 4], key: two ints -> uint32 [..., 4]."""
    c = [np.asarray(ctr, np.uint32)[..., k].astype(np.uint64) for k in range(4)]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(MASK), p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def uniform(words, lo, hi):
    """min(hi, lo + u (hi - lo)), u = (word >> 8) 2^-24, in float32 throughout."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    u = (np.asarray(words, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return np.minimum(hi, (lo + (u * (hi - lo)).astype(np.float32)).astype(np.float32)).astype(np.float32)


def _key(seed):
    seed = int(seed) & (2 ** 64 - 1)
    return seed & MASK, seed >> 32


def _words(seed, gids, second, stream, count):
    """`count` consecutive words of (gid, second, stream, block 0..) for every gid: uint32 [n, count]."""
    gids, second = np.asarray(gids, np.uint32), np.broadcast_to(np.asarray(second, np.uint32), np.shape(gids))
    nblk = (count + 3) // 4
    ctr = np.zeros((len(gids), nblk, 4), np.uint32)
    ctr[..., 0] = gids[:, None]; ctr[..., 1] = second[:, None]; ctr[..., 2] = stream; ctr[..., 3] = np.arange(nblk, dtype=np.uint32)[None, :]
    return philox4x32_10(ctr, _key(seed)).reshape(len(gids), 4 * nblk)[:, :count]


def sample_start(spec, gids, episodes):
    """(qpos0 float32 [n, nq], mocap float32 [n, 3], half yaw float32 [n, nblock]) of episode `episodes[i]` of global env `gids[i]`, for an
    episodes.EpisodeSpec.  The block quaternion is float32(cos / sin) of the float32 half yaw computed in float64."""
    gids = np.asarray(gids, np.uint32)
    nq = len(spec.qpos_lo)
    q = uniform(_words(spec.seed, gids, episodes, STREAM_QPOS, nq), spec.qpos_lo, spec.qpos_hi)
    nb = len(spec.block_qadr)
    half = np.zeros((len(gids), nb), np.float32)
    if nb:
        ep = np.broadcast_to(np.asarray(episodes, np.uint32), gids.shape)
        ctr = np.zeros((len(gids), nb, 4), np.uint32)
        ctr[..., 0] = gids[:, None]; ctr[..., 1] = ep[:, None]; ctr[..., 2] = STREAM_BLOCK; ctr[..., 3] = np.arange(nb, dtype=np.uint32)[None, :]
        pose = uniform(philox4x32_10(ctr, _key(spec.seed)), spec.block_lo, spec.block_hi)          # [n, nb, 4]
        half = (pose[..., 3] * np.float32(0.5)).astype(np.float32)
        for b, a in enumerate(spec.block_qadr):
            q[:, a:a + 3] = pose[:, b, :3]
            q[:, a + 3] = np.cos(half[:, b].astype(np.float64)); q[:, a + 4] = 0; q[:, a + 5] = 0
            q[:, a + 6] = np.sin(half[:, b].astype(np.float64))
    if spec.has_goal:
        g = uniform(_words(spec.seed, gids, episodes, STREAM_GOAL, 3), spec.goal_lo, spec.goal_hi)
    else:
        g = np.zeros((len(gids), 3), np.float32)
    return q, g, half


def sample_ctrl(seed, gids, step, ctrlrange):
    """ctrl float32 [n, nu] of action step `step`; a side of the range that is not finite or is the models' marker 1e30 counts as -1 / +1."""
    cr = np.asarray(ctrlrange, np.float32)
    lo = np.where(np.abs(cr[:, 0]) < np.float32(1e30), cr[:, 0], np.float32(-1)).astype(np.float32)
    hi = np.where(np.abs(cr[:, 1]) < np.float32(1e30), cr[:, 1], np.float32(1)).astype(np.float32)
    return uniform(_words(seed, gids, int(step) & MASK, STREAM_CTRL, len(cr)), lo, hi)


class Books:
    """The per-env books of hsr_batch_episode_end_dev for global envs `gids`."""

    def __init__(self, spec, gids):
        self.spec, self.gids = spec, np.asarray(gids, np.uint32)
        n = len(self.gids)
        self.index = np.zeros(n, np.uint32); self.length = np.zeros(n, np.int32); self.ret = np.zeros(n, np.float32)

    def begin(self, mask=None):
        """reset_sampled: (mask, qpos0, mocap, half yaw) - sample rows of unmasked envs are meaningless."""
        m = np.ones(len(self.gids), bool) if mask is None else np.asarray(mask, bool)
        q, g, half = sample_start(self.spec, self.gids, self.index)
        self.index[m] += 1; self.length[m] = 0; self.ret[m] = 0
        return m, q, g, half

    def end(self, reward, done):
        """After an env-step: (kind uint8 [n], fin_return, fin_length, qpos0, mocap) with samples for the envs of kind != 0."""
        done = np.asarray(done, bool)
        self.ret = (self.ret + np.asarray(reward, np.float32)).astype(np.float32)
        self.length = self.length + 1
        over = (self.spec.max_episode_steps > 0) & (self.length >= self.spec.max_episode_steps)
        kind = np.where(done, 1, np.where(over, 2, 0)).astype(np.uint8)
        sel = kind != 0
        fin_r, fin_l = np.where(sel, self.ret, 0).astype(np.float32), np.where(sel, self.length, 0).astype(np.int32)
        q, g, _ = sample_start(self.spec, self.gids, self.index)
        self.index[sel] += 1; self.length[sel] = 0; self.ret[sel] = 0
        return kind, fin_r, fin_l, q, g
