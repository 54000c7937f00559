"""Hindsight experience replay on the device (include/hsrsim.h: hsr_replay; DESIGN.md "Hindsight replay on the device").

The reference's task is sparse-reward and goal-conditioned - ``reward = float(block within geofence of a sampled point)``
(hsr/env.py:124-133), a new point every episode (hsr/env.py:161-172), observations meant as ``Obs(observation, goal)`` (hsr/env.py:275) -
and its host ring (rl_utils/replay_buffer.py:27-82) knows nothing of episodes.  ``HindsightReplay`` keeps the transitions of every env of a
``BatchSim`` on the device, episode by episode, and draws minibatches whose goals are relabelled with the 'future' strategy (Andrychowicz
et al., "Hindsight Experience Replay", NIPS 2017) and whose reward and done are recomputed by the env's own goal test.  Nothing visits
the host; a minibatch is a pure function of (seed, draw counter, ring contents).

``prioritized=True`` adds prioritised experience replay (Schaul et al., ICLR 2016) on a sum tree on the device (DESIGN.md "Prioritised
hindsight replay"): samples are drawn with probability priority / total, come with importance weights, and ``update_priorities`` stores
(|td| + eps)^alpha.  The transcendentals are torch ops on [B] tensors; the kernels only clamp, add and search.

Plumbing only: the kernels are csrc/replay.h and csrc/replay_prio.h.  There is no CPU stand-in.
"""
from __future__ import annotations

import torch

from .device_loop import batch_stream, zero_tensors
from .sim import BatchSim, PrioritySpec, ReplaySeqOut, ReplaySpec


class HindsightReplay:
    """Ring of the last `capacity_steps` transitions of every env of `sim`.

    Per env-step: ``record(ctrl, next_obs, reward, done)`` after ``sim.step_dev`` and before ``sim.episode_end_dev`` / any reset (the goal
    body's position is read from the batch at that moment), then ``commit(obs, reset)`` with the observation the policy acts on next and
    the envs that start a new episode with it.  ``sample(batch_size)`` and ``sample_sequences(batch_size, seq_len)`` may run whenever no
    record waits for its commit.
    Arguments are torch tensors on the batch's device (float32, uint8 for done / reset; reward / done None: what the step latched).

    prioritized=True: a transition's priority is (|td| + eps)^alpha, stored clamped into [eps^alpha, p_max]; a new transition enters with
    the largest priority stored so far (1 at first).  `max_batch` bounds the batch of a sample or an update."""

    def __init__(self, sim: BatchSim, capacity_steps: int, goal_body: int, geofence: float, obs_dim: int = None, her_ratio: float = 0.8,
                 seed: int = 0, env_offset: int = 0, prioritized: bool = False, alpha: float = 0.6, eps: float = 1e-6, p_max: float = 1e6,
                 max_batch: int = 4096):
        if not 0.0 <= float(her_ratio) <= 1.0:
            raise ValueError("her_ratio must lie in [0, 1]")
        if prioritized and not (float(alpha) >= 0.0 and float(eps) > 0.0):
            raise ValueError("prioritized replay needs alpha >= 0 and eps > 0")
        self.sim, self.her_ratio = sim, float(her_ratio)
        self.capacity_steps, self.obs_dim = int(capacity_steps), int(sim.nq + sim.nv if obs_dim is None else obs_dim)
        spec = ReplaySpec(seed=int(seed) & (2 ** 64 - 1), env_offset=int(env_offset) & 0xffffffff, capacity_steps=self.capacity_steps,
                          obs_dim=self.obs_dim, goal_body=int(goal_body), geofence=float(geofence))
        self._replay = sim.replay(spec)
        self._device, self._stream = batch_stream(sim)
        self._buffers = {}             # batch size -> the output tensors, allocated once
        self._seq_buffers = {}         # (batch size, seq_len) -> the output tensors of sample_sequences
        self._draw = 0
        self.prioritized, self.alpha, self.eps = bool(prioritized), float(alpha), float(eps)
        self._pushed = 0               # the library's 64-bit `pushed`, followed through its low word (_token)
        if self.prioritized:
            p_min = min(self.eps ** self.alpha, 1.0)
            self._replay.priority_enable(PrioritySpec(p_init=1.0, p_min=p_min, p_max=max(float(p_max), 1.0), max_batch=int(max_batch)))

    def _ptr(self, t, shape, dtype):
        if t is None:
            return None
        if tuple(t.shape) != shape or str(t.dtype) != dtype or not t.is_contiguous() or t.device != self._device:
            raise AssertionError(f"replay: expected a contiguous {dtype} tensor of shape {shape} on {self._device}")
        return t.data_ptr()

    def commit(self, obs, reset=None):
        n = self.sim.n
        self._replay.commit_dev(self._ptr(obs, (n, self.obs_dim), "torch.float32"), self._ptr(reset, (n,), "torch.uint8"))

    def record(self, ctrl, next_obs, reward=None, done=None):
        n = self.sim.n
        self._replay.record_dev(self._ptr(ctrl, (n, self.sim.nu), "torch.float32"), self._ptr(next_obs, (n, self.obs_dim), "torch.float32"),
                                self._ptr(reward, (n,), "torch.float32"), self._ptr(done, (n,), "torch.uint8"))

    def _token(self):
        """`pushed` as 64 bits, from the host books (no device work): the sampled_at token of a sample taken now."""
        self._pushed += (self._replay.state()[2] - self._pushed) & 0xffffffff
        return self._pushed

    def _weigh(self, out, beta):
        """weight = (count N prob)^-beta / its maximum over the batch, on the replay's stream after the sample."""
        with torch.cuda.stream(self._stream):
            w = (out["prob"] * float(len(self))) ** (-float(beta))
            torch.div(w, w.max(), out=out["weight"])
        out["sampled_at"] = self._token()

    def sample(self, batch_size: int, beta: float = 0.4, normalizer=None) -> dict:
        """The next minibatch: obs [B, obs_dim], action [B, nu], next_obs, goal [B, 3], achieved_next [B, 3], reward [B] (float32), done [B]
        (uint8) and index [B, 4] (int32: env, slot, goal slot or -1, relabelled), written on the batch's stream into tensors that the next
        sample() of the same size overwrites.  Order torch work after it with ``torch.cuda.stream(replay.stream)`` or a stream wait.
        A prioritised replay draws by priority and adds prob [B] (priority / total), weight [B] ((count N prob)^-beta over its maximum in the
        batch) and sampled_at (an int: hand it, or the whole dict, to update_priorities).
        normalizer (normalize.ObsNormalizer): its ``apply_batch`` normalises the drawn rows in place, in one more launch; the ring keeps
        raw rows.  None: nothing more runs."""
        b = int(batch_size)
        out = self._buffers.get(b)
        if out is None:
            f32 = torch.float32
            extra = dict(prob=((b,), f32), weight=((b,), f32)) if self.prioritized else {}
            out = self._buffers[b] = zero_tensors(self._device, dict(
                obs=((b, self.obs_dim), f32), action=((b, self.sim.nu), f32), next_obs=((b, self.obs_dim), f32), goal=((b, 3), f32),
                achieved_next=((b, 3), f32), reward=((b,), f32), done=((b,), torch.uint8), index=((b, 4), torch.int32), **extra))
        p = {k: v.data_ptr() for k, v in out.items() if k != "sampled_at"}
        if self.prioritized:
            self._replay.priority_sample_dev(self._draw, b, self.her_ratio, p["obs"], p["action"], p["next_obs"], p["goal"], p["achieved_next"],
                                             p["reward"], p["done"], p["index"], p["prob"])
            self._weigh(out, beta)
        else:
            self._replay.sample_dev(self._draw, b, self.her_ratio, p["obs"], p["action"], p["next_obs"], p["goal"], p["achieved_next"], p["reward"],
                                    p["done"], p["index"])
        self._draw = (self._draw + 1) & 0xffffffff
        if normalizer is not None:
            normalizer.apply_batch(out)
        return out

    def sample_sequences(self, batch_size: int, seq_len: int, gamma: float = 0.99, beta: float = 0.4, normalizer=None) -> dict:
        """The next minibatch as windows of up to `seq_len` steps, for recurrent policies and n-step targets: the sampled step and the
        steps after it inside its episode (never past the episode's end or the ring's newest step), all under one goal - the desired one,
        or the achieved goal of a later step of the episode for a relabelled sample.  With L = seq_len: obs [B, L, obs_dim], action
        [B, L, nu], next_obs, achieved_next [B, L, 3], reward [B, L], done [B, L] (uint8), zero past ``length`` [B] (int32, 1..L); goal
        [B, 3]; index [B, 4] as in sample(), for the first step.  ``nstep`` [B] = m, the steps up to and including the first done one
        (else ``length``), ``nstep_return`` = sum of gamma^k reward_k over them, ``nstep_discount`` = gamma^m, ``nstep_obs`` [B, obs_dim]
        = next_obs of step m-1, ``nstep_done`` [B] (uint8).  A window cut by the time limit, by L or by the ring's newest step has
        nstep_done = 0: bootstrap from nstep_obs, target = nstep_return + nstep_discount (1 - nstep_done) V(nstep_obs, goal).
        Tensors are written on the batch's stream and overwritten by the next call of the same (batch_size, seq_len); the draw counter is
        the one sample() advances.  A prioritised replay draws the window's first step by priority and adds prob, weight and sampled_at as
        sample() does.  normalizer: as in sample(); the padding rows past ``length`` stay zero."""
        b, n = int(batch_size), int(seq_len)
        out = self._seq_buffers.get((b, n))
        if out is None:
            f32, u8, i32 = torch.float32, torch.uint8, torch.int32
            out = self._seq_buffers[(b, n)] = zero_tensors(self._device, dict(
                obs=((b, n, self.obs_dim), f32), action=((b, n, self.sim.nu), f32), next_obs=((b, n, self.obs_dim), f32),
                achieved_next=((b, n, 3), f32), goal=((b, 3), f32), reward=((b, n), f32), done=((b, n), u8), length=((b,), i32), nstep=((b,), i32),
                nstep_return=((b,), f32), nstep_discount=((b,), f32), nstep_obs=((b, self.obs_dim), f32), nstep_done=((b,), u8),
                index=((b, 4), i32), **(dict(prob=((b,), f32), weight=((b,), f32)) if self.prioritized else {})))
        ptr = {"act" if k == "action" else k: v.data_ptr() for k, v in out.items() if k not in ("prob", "weight", "sampled_at")}
        if self.prioritized:
            self._replay.priority_sample_seq_dev(self._draw, b, n, self.her_ratio, gamma, ReplaySeqOut(**ptr), out["prob"].data_ptr())
            self._weigh(out, beta)
        else:
            self._replay.sample_seq_dev(self._draw, b, n, self.her_ratio, gamma, ReplaySeqOut(**ptr))
        self._draw = (self._draw + 1) & 0xffffffff
        if normalizer is not None:
            normalizer.apply_batch(out)
        return out

    def update_priorities(self, batch_or_index, td_error, sampled_at: int = None):
        """Store (|td_error| + eps)^alpha as the priority of every sampled cell: `batch_or_index` is the dict a sample returned (its
        sampled_at is used) or its index tensor [B, 4]; td_error float [B] on the device.  Rows whose cell was overwritten since the
        sample are skipped; of rows that name one cell the largest priority wins.  Runs on the replay's stream, after the work queued on
        torch's current stream."""
        if not self.prioritized:
            raise ValueError("update_priorities on a replay made without prioritized=True")
        if isinstance(batch_or_index, dict):
            index = batch_or_index["index"]
            sampled_at = batch_or_index["sampled_at"] if sampled_at is None else sampled_at
        else:
            index = batch_or_index
        if sampled_at is None:
            sampled_at = self._token()
        b = int(index.shape[0])
        self._ptr(index, (b, 4), "torch.int32")
        self._stream.wait_stream(torch.cuda.current_stream(self._device))
        with torch.cuda.stream(self._stream):
            prio = ((td_error.detach().reshape(b).to(torch.float32).abs() + self.eps) ** self.alpha).contiguous()
            self._replay.priority_update_dev(int(sampled_at), b, index.data_ptr(), prio.data_ptr())

    def priority_state(self):
        """(pushed, total priority, priority of a new transition); synchronises the replay's stream."""
        return self._replay.priority_state()

    @property
    def stream(self):
        """The batch's stream as a torch stream: where record / commit / sample run."""
        return self._stream

    def state(self):
        """(count, head slot, pushed & 0xffffffff) from the host books."""
        return self._replay.state()

    def clear(self):
        """Forget every transition and episode (the storage stays); the next call must be commit()."""
        self._replay.clear()
        self._pushed = 0

    def close(self):
        self._replay.close()
        self._buffers, self._seq_buffers = {}, {}

    def __len__(self):
        return self._replay.state()[0] * self.sim.n


__all__ = ["HindsightReplay", "ReplaySpec"]
