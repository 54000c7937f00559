"""Checker-side restatement of the device replay's window sampler (include/hsrsim.h: hsr_replay_sample_seq_dev), in numpy, written from
its specification on top of replay_ref.Ring: the draw and the episode's last age are Ring.indices, the window is the ages j .. j + length
- 1, one goal serves the whole window, and the n-step reduction takes each float32 operation on its own.  The product never imports it.

Rows are copied, never computed on, so bit patterns survive; padding is zero words.  The float computations are the relabelled reward
(replay_ref.within, operation by operation) and the n-step chain: term = g * reward_k, acc = acc + term, g = g * gamma, each rounded to
float32 before the next."""
import numpy as np

from replay_ref import OutOfOrder, within

PER_STEP = ("obs", "action", "next_obs", "achieved_next", "reward", "done")
PER_SAMPLE = ("goal", "length", "nstep", "nstep_return", "nstep_discount", "nstep_obs", "nstep_done", "index")
SEQ_FIELDS = ("obs", "action", "next_obs", "achieved_next", "goal", "reward", "done", "length", "nstep", "nstep_return", "nstep_discount", "nstep_obs",
              "nstep_done", "index")


def nstep(reward, done, length, gamma):
    """(m, acc, g, done_{m-1}) of one window: reward [L] float32, done [L], the first `length` entries valid."""
    gamma, acc, g = np.float32(gamma), np.float32(0), np.float32(1)
    m = 0
    for k in range(int(length)):
        term = np.float32(g * np.float32(reward[k]))
        acc = np.float32(acc + term)
        g = np.float32(g * gamma)
        m = k + 1
        if done[k] != 0:
            break
    return m, acc, g, np.uint8(done[m - 1] != 0)


def sample_seq(ring, draw, batch, seq_len, her_ratio, gamma):
    """The arrays hsr_replay_sample_seq_dev writes for (draw, batch, seq_len, her_ratio, gamma), keyed as HindsightReplay.sample_sequences."""
    L = int(seq_len)
    g32 = np.float32(gamma)
    if L < 1 or L > ring.T or not np.isfinite(g32) or g32 < 0 or g32 > 1 or batch * L >= 2 ** 31:
        raise OutOfOrder("sample_seq")
    e, j, relabel, j_end, j_goal = ring.indices(draw, batch, her_ratio)
    length = np.minimum(L, j_end - j + 1)
    steps = np.arange(L, dtype=np.int64)
    valid = steps[None, :] < length[:, None]                                        # [batch, L]
    age = np.where(valid, j[:, None] + steps[None, :], j[:, None])                  # a padded step reads nothing: any stored age will do
    s, env = ring.slot(age), np.broadcast_to(e[:, None], age.shape)
    sj, sg = ring.slot(j), ring.slot(j_goal)
    goal = np.where(relabel[:, None], ring.achieved[sg, e], ring.desired[sj, e]).astype(np.float32)

    def rows(a):
        got = a[s, env].copy()
        got[~valid] = 0
        return got

    achieved = ring.achieved[s, env]
    reach = within(achieved, goal[:, None, :], ring.geofence)
    reward = np.where(relabel[:, None], reach.astype(np.float32), ring.reward[s, env]).astype(np.float32)
    done = np.where(relabel[:, None], reach, ring.done[s, env] != 0).astype(np.uint8)
    reward[~valid] = 0
    done[~valid] = 0
    m, ret, disc, ndone = np.zeros(batch, np.int32), np.zeros(batch, np.float32), np.zeros(batch, np.float32), np.zeros(batch, np.uint8)
    for i in range(batch):
        m[i], ret[i], disc[i], ndone[i] = nstep(reward[i], done[i], length[i], gamma)
    last = ring.slot(j + m - 1)
    index = np.stack([e, sj, np.where(relabel, sg, -1), relabel.astype(np.int64)], axis=1).astype(np.int32)
    return dict(obs=rows(ring.obs), action=rows(ring.act), next_obs=rows(ring.next_obs), achieved_next=rows(ring.achieved), goal=goal, reward=reward,
                done=done, length=length.astype(np.int32), nstep=m, nstep_return=ret, nstep_discount=disc, nstep_obs=ring.next_obs[last, e],
                nstep_done=ndone, index=index)
