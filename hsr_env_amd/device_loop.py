"""The device loop of ``VecHSREnv(auto_reset=True)``: the torch and device-pointer plumbing around ``BatchSim``'s ``*_dev`` calls.

``DeviceLoop`` owns the batch's stream as a torch stream, the tensors a step reads and writes, the action-step counter of the device's
action sampler and the attached ``replay.HindsightReplay``.  ``DeviceLoop.step`` is the one place where the order of the library calls
of an env-step - step, record, episode end, commit - is written.  The env keeps the gym surface and the host books.

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
    def __init__(self, sim, n_envs: int, nu: int, state_dim: int, obs_dim: int):
        self.sim, self.n, self.nu, self.state_dim, self.obs_dim = sim, n_envs, nu, state_dim, obs_dim
        self.action_step = 0           # the next draw of sample_action(); part of an env's saved state
        self.replay = None
        self._buf = None               # the stream and the tensors, made at the first use (and again when a replay is attached)

    def _buffers(self):
        if self._buf is None:
            n, f32, u8, i32 = self.n, torch.float32, torch.uint8, torch.int32
            table = dict(ctrl=((n, self.nu), f32), obs=((n, self.state_dim), f32), final=((n, self.state_dim), f32), rew=((n,), f32),
                         fret=((n,), f32), done=((n,), u8), kind=((n,), u8), ns=((n,), i32), flen=((n,), i32))
            if self.replay is not None:                                 # rows handed to the replay that no other buffer holds
                table.update(robs=((n, self.obs_dim), f32), rmask=((n,), u8))
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
        sim, replay = self.sim, self.replay
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
            if replay is not None:
                if openai:
                    sim.obs_openai_dev(ptr["robs"])
                replay.record(d["ctrl"], d["robs"] if openai else d["obs"], d["rew"], d["done"])
            sim.episode_end_dev(ptr["obs"], ptr["rew"], ptr["done"], None if openai else ptr["final"], ptr["kind"], ptr["fret"], ptr["flen"])
            if replay is not None:
                if openai:
                    sim.obs_openai_dev(ptr["robs"])                     # the first observation of the envs that were reset
                replay.commit(d["robs"] if openai else d["obs"], d["kind"])
            host = {k: d[k].cpu().numpy() for k in ("obs", "rew", "done", "ns", "kind", "fret", "flen")}
            if not openai:
                terminal = d["final"].cpu().numpy()
        return StepRecord(host["obs"], host["rew"], host["done"], host["ns"], host["kind"], host["fret"], host["flen"], terminal)

    # ------------------------------------------------------------------ the replay the loop feeds
    def attach_replay(self, replay):
        self.replay = replay
        self._buf = None                                                # the buffers gain the replay's staging rows

    def commit_host_rows(self, obs, mask=None):
        """commit() of host rows: the observation reset() returns, and the envs it began an episode for (None: all of them)."""
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
        """After a jump (load_state, fork) the ring describes a past the envs no longer have: forget it and start from the current rows."""
        if self.replay is not None:
            self.replay.clear()
            self.commit_host_rows(obs)
