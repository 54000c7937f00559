"""On-policy rollouts on the device (include/hsrsim.h: hsr_rollout; DESIGN.md "On-policy rollouts on the device").

A batch of lock-stepped envs is the regime of PPO / A2C.  ``OnPolicyRollout`` keeps `horizon` env-steps of every env of a ``BatchSim`` on
the device - observation, action, log-probability, value, reward, reset kind - and, once the horizon is reached, computes generalised
advantage estimates (Schulman et al., "High-Dimensional Continuous Control Using Generalized Advantage Estimation", ICLR 2016) with the
bootstrap a time limit calls for (the value of the TERMINAL observation where the episode was cut, nothing where it ended), the
advantages' mean and deviation, and shuffled minibatches.  Nothing visits the host; a minibatch is a pure function of
(seed, epoch, position, contents).

Plumbing only: the kernels are csrc/rollout.h.  There is no CPU stand-in.
"""
from __future__ import annotations

import torch

from .device_loop import batch_stream, zero_tensors
from .sim import ROLLOUT_STAGED, BatchSim, RolloutSpec


class OnPolicyRollout:
    """`horizon` env-steps of every env of `sim`.

    Per env-step: ``stage(action, logp, value)`` with what the policy computed from ``obs``, then ``close_step(reward, kind, next_obs,
    terminal_obs)`` after ``sim.episode_end_dev`` (the env of ``VecHSREnv.make_rollout`` does the latter inside ``step``), then
    ``bootstrap(critic(terminal_obs))``.  After `horizon` steps ``finish(critic(obs))``, any number of ``minibatches(...)``, ``next()``.
    Arguments are torch tensors on the batch's device (float32; uint8 for kind).  The kernels run on the batch's stream: every call that
    reads tensors of the caller first makes that stream wait for torch's current one, and every call that hands tensors out makes torch's
    current stream wait for the batch's, so a loop written on torch's default stream needs no synchronisation of its own."""

    def __init__(self, sim: BatchSim, horizon: int, obs_dim: int = None, gamma: float = 0.99, lam: float = 0.95, seed: int = 0, env_offset: int = 0):
        self.sim, self.horizon, self.gamma, self.lam = sim, int(horizon), float(gamma), float(lam)
        self.obs_dim = int(sim.nq + sim.nv if obs_dim is None else obs_dim)
        spec = RolloutSpec(seed=int(seed) & (2 ** 64 - 1), env_offset=int(env_offset) & 0xffffffff, horizon=self.horizon, obs_dim=self.obs_dim,
                           gamma=self.gamma, lam=self.lam)
        self._rollout = sim.rollout(spec)
        self._device, self._stream = batch_stream(sim)
        self._buffers = {}             # batch size -> the output tensors, allocated once
        self._planes = None
        self.obs = None                # [N, obs_dim]: what the policy acts on now (the tensor handed to begin / close last)
        self.terminal_obs = None       # [N, obs_dim]: what the last step produced before its reset - the critic's input for bootstrap()

    def _ptr(self, t, shape, dtype):
        if tuple(t.shape) != shape or str(t.dtype) != dtype or not t.is_contiguous() or t.device != self._device:
            raise AssertionError(f"rollout: expected a contiguous {dtype} tensor of shape {shape} on {self._device}")
        return t.data_ptr()

    def _after_torch(self):
        """The batch's stream waits for what torch's current stream has queued (the tensors about to be read)."""
        cur = torch.cuda.current_stream(self._device)
        if cur != self._stream:
            self._stream.wait_stream(cur)

    def _before_torch(self):
        """torch's current stream waits for the batch's (the tensors just written)."""
        cur = torch.cuda.current_stream(self._device)
        if cur != self._stream:
            cur.wait_stream(self._stream)

    def _vec(self, t):
        """A per-env float32 value, [N] or [N, 1]."""
        if t.dim() == 2 and t.shape[1] == 1:
            t = t.reshape(-1)
        return self._ptr(t, (self.sim.n,), "torch.float32")

    def begin(self, obs):
        """Start (again) from `obs`: the rollout is empty and the policy acts on these rows next."""
        self._after_torch()
        self._rollout.begin_dev(self._ptr(obs, (self.sim.n, self.obs_dim), "torch.float32"))
        self.obs, self.terminal_obs = obs, None

    def stage(self, action, logp, value):
        self._after_torch()
        self._rollout.stage_dev(self._ptr(action, (self.sim.n, self.sim.nu), "torch.float32"), self._vec(logp), self._vec(value))

    def close_step(self, reward, kind, next_obs, terminal_obs=None):
        """Close the staged step: its reward and reset kind (0 goes on, 2 cut by the time limit, else ended), and the rows the policy acts on
        next; `terminal_obs` is kept for the caller's critic."""
        n = self.sim.n
        self._after_torch()
        self._rollout.close_dev(self._ptr(reward, (n,), "torch.float32"), self._ptr(kind, (n,), "torch.uint8"),
                                self._ptr(next_obs, (n, self.obs_dim), "torch.float32"))
        self.obs, self.terminal_obs = next_obs, terminal_obs

    def bootstrap(self, value_terminal):
        """The critic's value of ``terminal_obs`` for every env; used where the step closed last was cut by the time limit."""
        self._after_torch()
        self._rollout.bootstrap_dev(self._vec(value_terminal))

    def finish(self, last_value):
        """``last_value = critic(obs)`` after the last step: advantages, returns and their statistics are computed on the batch's stream."""
        self._after_torch()
        self._rollout.finish_dev(self._vec(last_value))

    def minibatches(self, batch_size: int, epoch: int, normalize: bool = True):
        """The shuffle of `epoch` cut into minibatches: dicts of obs [B, obs_dim], action [B, nu], logp, value, advantage, ret [B] (float32)
        and index [B, 2] (int32: step, env); the last one of an epoch may be shorter.  The tensors are views of buffers that the next
        minibatch of the same batch size overwrites."""
        b, total = int(batch_size), self.horizon * self.sim.n
        if b < 1:
            raise ValueError("batch_size < 1")
        out = self._buffers.get(b)
        if out is None:
            f32 = torch.float32
            out = self._buffers[b] = zero_tensors(self._device, dict(
                obs=((b, self.obs_dim), f32), action=((b, self.sim.nu), f32), logp=((b,), f32), value=((b,), f32), advantage=((b,), f32),
                ret=((b,), f32), index=((b, 2), torch.int32)))
        p = {k: v.data_ptr() for k, v in out.items()}
        for first in range(0, total, b):
            count = min(b, total - first)
            self._after_torch()                                         # whoever still reads the previous minibatch
            self._rollout.minibatch_dev(epoch, first, count, normalize, p["obs"], p["action"], p["logp"], p["value"], p["advantage"], p["ret"], p["index"])
            self._before_torch()
            yield {k: v[:count] for k, v in out.items()}

    def _plane(self, which):
        if self._planes is None:
            shape = (self.horizon, self.sim.n)
            self._planes = zero_tensors(self._device, dict(adv=(shape, torch.float32), ret=(shape, torch.float32)))
        self._after_torch()
        self._rollout.planes_dev(**{"d_" + which: self._planes[which].data_ptr()})
        self._before_torch()
        return self._planes[which]

    def advantages(self):
        """[T, N] float32, not normalised; a buffer of this object that the next call overwrites."""
        return self._plane("adv")

    def returns(self):
        return self._plane("ret")

    def stats(self):
        """(mean, std, 1 / (std + 1e-8)) of the advantages, float32 as the device keeps them; synchronises."""
        return self._rollout.stats()

    def next(self):
        """The finished rollout is used up: the next one starts from the current ``obs``."""
        self._rollout.next()

    @property
    def staged(self) -> bool:
        return self._rollout.state()[0] == ROLLOUT_STAGED

    @property
    def stream(self):
        """The batch's stream as a torch stream: where every call of this object runs."""
        return self._stream

    def state(self):
        """(state: 0 empty, 1 ready, 2 staged, 3 done; steps closed) from the host books."""
        return self._rollout.state()

    def close(self):
        """Release the device storage (the batch's close() does so too)."""
        self._rollout.close()
        self._buffers, self._planes = {}, None


__all__ = ["OnPolicyRollout", "RolloutSpec"]
