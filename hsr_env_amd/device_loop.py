"""The device loop of ``VecHSREnv(auto_reset=True)``: the torch and device-pointer plumbing around ``BatchSim``'s ``*_dev`` calls.

``DeviceLoop`` owns the batch's stream as a torch stream, the tensors a step reads and writes, the action-step counter of the device's
action sampler and the attached ``replay.HindsightReplay``, ``rollout.OnPolicyRollout`` and ``normalize.ObsNormalizer`` (any of them or
none; they do not know of each other).  ``DeviceLoop.step`` is the one place where the order of the library calls of an env-step - step,
record, episode end, commit, close, observe - is written.  The env keeps the gym surface and the host books.

Importing this module imports torch; ``VecHSREnv`` does so only with ``auto_reset=True``.  There is no CPU stand-in.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from .sim import raise_if_diverged

# what one env-step hands to the host (numpy, one row per env).  kind: 0 the episode goes on, 1 it ended in done, 2 it ran out of time;
# fin_return / fin_length describe the episode that ended; terminal_obs is what the step produced before the reset moved the envs
StepRecord = namedtuple("StepRecord", "obs reward done nsteps kind fin_return fin_length terminal_obs")


def batch_stream(sim):
    """(the torch device of a batch, the batch's stream as a torch stream)."""
    device = torch.device("cuda", getattr(sim, "device", 0))
    return device, torch.cuda.ExternalStream(sim.stream_ptr(), device=device)


def zero_tensors(device, table):
    """{name: (shape, dtype)} -> {name: zero tensor}, ready for the batch's stream."""
    out = {name: torch.zeros(shape, dtype=dtype, device=device) for name, (shape, dtype) in table.items()}
    torch.cuda.synchronize(device)                                      # the fills ran on torch's stream, the batch has its own
    return out


class DeviceLoop:
    def __init__(self, sim, n_envs: int, nu: int, state_dim: int, obs_dim: int, openai: bool = False):
        self.sim, self.n, self.nu, self.state_dim, self.obs_dim = sim, n_envs, nu, state_dim, obs_dim
        self.openai = bool(openai)     # the env's rows are the 25-float observation, which no step output holds
        self.action_step = 0           # the next draw of sample_action(); part of an env's saved state
        self.replay = None
        self.rollout = None
        self.normalizer = None
        self._buf = None               # the stream and the tensors, made at the first use (and again when something is attached)

    def _buffers(self):
        if self._buf is None:
            n, f32, u8, i32 = self.n, torch.float32, torch.uint8, torch.int32
            table = dict(ctrl=((n, self.nu), f32), obs=((n, self.state_dim), f32), final=((n, self.state_dim), f32), rew=((n,), f32),
                         fret=((n,), f32), done=((n,), u8), kind=((n,), u8), ns=((n,), i32), flen=((n,), i32))
            # rows handed to the replay and the rollout that no other buffer holds: the policy rows (robs: the observation as the env
            # returns it; with the state observation `obs` serves the rollout) and, for the 25-float observation, the terminal rows
            if self.replay is not None or (self.openai and (self.rollout is not None or self.normalizer is not None)):
                table.update(robs=((n, self.obs_dim), f32), rmask=((n,), u8))
            elif self.normalizer is not None:
                table.update(rmask=((n,), u8))
            if self.rollout is not None and self.openai:
                table.update(rterm=((n, self.obs_dim), f32))
            device, stream = batch_stream(self.sim)
            self._buf = stream, zero_tensors(device, table)
        return self._buf

    def sample_action(self):
        """Uniform actions over the action space drawn on the device (torch float32 [n_envs, nu]); every call is the next action step."""
        stream, d = self._buffers()
        with torch.cuda.stream(stream):
            self.sim.sample_ctrl_dev(self.action_step, d["ctrl"].data_ptr())
        self.action_step += 1
        return d["ctrl"]

    def restart(self, spec):
        """seed(): the device samplers - episodes and actions - start again from `spec` (episodes.EpisodeSpec)."""
        self.sim.set_episodes(spec)
        self.action_step = 0

    def reset(self, mask):
        """The masked envs draw their next episode."""
        self.sim.reset_sampled(mask)

    def step(self, action, steps, goal_body, geofence, openai, recorder) -> StepRecord:
        """One env-step with the episode end inside it.  ``action``: host rows, or a torch tensor on the device (the tensor of
        sample_action() is used in place)."""
        sim, replay, rollout = self.sim, self.replay, self.rollout
        if rollout is not None and not rollout.staged:
            raise ValueError("step() of an env that feeds a rollout needs rollout.stage(action, logp, value) first: the step would be lost to it")
        stream, d = self._buffers()
        ptr = {k: v.data_ptr() for k, v in d.items()}
        with torch.cuda.stream(stream):
            if not isinstance(action, torch.Tensor):
                d["ctrl"].copy_(torch.from_numpy(np.ascontiguousarray(action, dtype=np.float32).reshape(self.n, self.nu)))
            elif action.data_ptr() != ptr["ctrl"]:
                d["ctrl"].copy_(action.reshape(self.n, self.nu))
            sim.step_dev(ptr["ctrl"], steps, goal_body, geofence, ptr["obs"], ptr["rew"], ptr["done"], ptr["ns"])
            raise_if_diverged(sim)
            if recorder is not None:
                recorder.after_step(d["done"].cpu().numpy().astype(bool), d["ns"].cpu().numpy())
            # before the reset moves the bodies: the terminal rows, and the achieved goal the replay reads from the poses of this step
            terminal = sim.obs_openai() if openai else None
            fed = replay is not None or rollout is not None
            term_rows, policy_rows = (d["rterm" if rollout is not None else "robs"], d["robs"]) if openai and fed else (d["final"], d["obs"])
            if openai and fed:
                sim.obs_openai_dev(term_rows.data_ptr())
            if replay is not None:
                replay.record(d["ctrl"], term_rows if openai else d["obs"], d["rew"], d["done"])
            sim.episode_end_dev(ptr["obs"], ptr["rew"], ptr["done"], None if openai else ptr["final"], ptr["kind"], ptr["fret"], ptr["flen"])
            if openai and self.normalizer is not None and not fed:
                policy_rows = d["robs"]                                 # nothing else asked for the policy rows of this observation
            if openai and (fed or self.normalizer is not None):
                sim.obs_openai_dev(policy_rows.data_ptr())              # the first observation of the envs that were reset
            if replay is not None:
                replay.commit(policy_rows, d["kind"])
            if rollout is not None:                                     # after the replay's commit; neither reads what the other wrote
                rollout.close_step(d["rew"], d["kind"], policy_rows, term_rows)
            if self.normalizer is not None:                             # the last link: the rows the policy acts on next, counted once
                self.normalizer.observe(policy_rows)
            host = {k: d[k].cpu().numpy() for k in ("obs", "rew", "done", "ns", "kind", "fret", "flen")}
            if not openai:
                terminal = d["final"].cpu().numpy()
        return StepRecord(host["obs"], host["rew"], host["done"], host["ns"], host["kind"], host["fret"], host["flen"], terminal)

    # ------------------------------------------------------------------ the replay the loop feeds
    def attach_replay(self, replay):
        self.replay = replay
        self._buf = None                                                # the buffers gain the replay's staging rows

    def commit_host_rows(self, obs, mask=None, count=True):
        """The host rows of a reset() - the observation it returns, and the envs it began an episode for (None: all of them) - go to what the
        loop feeds: the replay commits them, the rollout begins again from them, the normaliser counts them.  count=False: rows the policy
        was handed before - make_replay committing the current rows to its new ring, a jump - are not counted a second time."""
        self.begin_rollout(obs)
        if count:
            self.observe_host_rows(obs, mask)
        if self.replay is None:
            return
        stream, d = self._buffers()
        with torch.cuda.stream(stream):
            d["robs"].copy_(torch.from_numpy(np.ascontiguousarray(obs, dtype=np.float32).reshape(self.n, self.obs_dim)))
            if mask is not None:
                d["rmask"].copy_(torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.n)))
            self.replay.commit(d["robs"], None if mask is None else d["rmask"])
            stream.synchronize()                                        # the host rows are pageable: the copies must not outlive them

    def restart_replay(self, obs):
        """After a jump (load_state, fork) the ring describes a past the envs no longer have: forget it and start from the current rows;
        so does the rollout.  The normaliser's statistics are the learner's and stay as they are."""
        if self.replay is not None:
            self.replay.clear()
        self.commit_host_rows(obs, count=False)
        self.observe_host_rows(obs, count=False)

    # ------------------------------------------------------------------ the rollout the loop feeds
    def attach_rollout(self, rollout):
        self.rollout = rollout
        self._buf = None                                                # the buffers gain the rollout's rows

    def begin_rollout(self, obs):
        """The rollout starts (again) from host rows - commit_host_rows calls this: the observation reset() returned, or the current one
        after a jump (load_state, fork); steps gathered before it describe a past the envs no longer have."""
        if self.rollout is None:
            return
        stream, d = self._buffers()
        rows = d["robs"] if self.openai else d["obs"]
        with torch.cuda.stream(stream):
            rows.copy_(torch.from_numpy(np.ascontiguousarray(obs, dtype=np.float32).reshape(self.n, self.obs_dim)))
            self.rollout.begin(rows)
            stream.synchronize()                                        # the host rows are pageable: the copy must not outlive them

    # ------------------------------------------------------------------ the normaliser the loop feeds
    def attach_normalizer(self, normalizer):
        """Nothing the loop already feeds is disturbed: tensors that exist stay, the ones the normaliser needs besides them - the reset mask,
        and the policy rows of the 25-float observation - are added."""
        self.normalizer = normalizer
        if self._buf is not None:
            stream, d = self._buf
            table = dict(rmask=((self.n,), torch.uint8), **(dict(robs=((self.n, self.obs_dim), torch.float32)) if self.openai else {}))
            d.update(zero_tensors(d["ctrl"].device, {k: v for k, v in table.items() if k not in d}))

    def observe_host_rows(self, obs, mask=None, count=True):
        """The normaliser counts the host rows of a reset() for the envs of `mask` (None: all) and normalises all of them into its
        ``policy_obs``.  count=False (after a jump): the statistics stay, policy_obs follows the rows."""
        if self.normalizer is None:
            return
        if not count:
            mask = np.zeros(self.n, dtype=np.uint8)
        stream, d = self._buffers()
        rows = d["robs"] if self.openai else d["obs"]
        with torch.cuda.stream(stream):
            rows.copy_(torch.from_numpy(np.ascontiguousarray(obs, dtype=np.float32).reshape(self.n, self.obs_dim)))
            if mask is not None:
                d["rmask"].copy_(torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.n)))
            self.normalizer.observe(rows, None if mask is None else d["rmask"])
            stream.synchronize()                                        # the host rows are pageable: the copies must not outlive them
