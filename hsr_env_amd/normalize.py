"""Running mean / std normalisation of observations and goals on the device (include/hsrsim.h: hsr_norm; DESIGN.md "Normalising
observations and goals on the device").

The state observation mixes slide positions in metres, a quaternion and joint velocities tens of times larger, and hindsight replay on a
sparse reward is known not to train without per-column normalisation and clipping (Andrychowicz et al., "Hindsight Experience Replay",
NIPS 2017, and the baselines' normalizer: eps = 0.01, clip = 5).  ``RunningNorm`` keeps count, mean and the sum of squared deviations of
every column in fp64 on the device, merges each batch of rows by Chan's rule with sums of a fixed shape - the same rows give the same bits,
run after run -, publishes float32 mean and 1 / std, and applies ``clamp((x - mean) / std, -clip, clip)`` in float32.  Rows with a NaN or
an infinity are left out and counted in ``skipped``: one diverged env does not poison the statistics.  Nothing visits the host.

``ObsNormalizer`` is the pair a goal-conditioned learner needs - one ``RunningNorm`` for the observation, one for the 3-float goal - and
what ``VecHSREnv.make_normalizer`` attaches to the device loop.

Plumbing only: the kernels are csrc/normalize.h.  There is no CPU stand-in.
"""
from __future__ import annotations

import numpy as np
import torch

from .device_loop import batch_stream, zero_tensors
from .sim import BatchSim, norm_apply_batch_dev


class RunningNorm:
    """Running moments of `dim` columns on the device of `sim`, and the normalisation they define.

    ``update(rows, mask)`` counts rows, ``apply(rows, out)`` normalises rows with the statistics of the moment.  Rows are float32 torch
    tensors on the batch's device whose last dimension is `dim`: two-dimensional ones may have any row stride (a column slice of a wider
    tensor), others must be contiguous.  Host numpy rows are accepted too and copied up (and, for apply, down again).  The kernels run on
    the batch's stream: a call first makes that stream wait for torch's current one and then torch's current one wait for it, so a loop
    written on torch's default stream needs no synchronisation of its own."""

    def __init__(self, sim: BatchSim, dim: int, eps: float = 0.01, clip: float = 5.0):
        self.sim, self.dim, self.eps, self.clip = sim, int(dim), float(np.float32(eps)), float(np.float32(clip))
        self._norm = sim.norm(self.dim, eps, clip)
        self._device, self._stream = batch_stream(sim)
        self._published = None

    # ------------------------------------------------------------------ streams and arguments
    def _after_torch(self):
        cur = torch.cuda.current_stream(self._device)
        if cur != self._stream:
            self._stream.wait_stream(cur)

    def _before_torch(self):
        cur = torch.cuda.current_stream(self._device)
        if cur != self._stream:
            cur.wait_stream(self._stream)

    def _rows(self, t, what):
        """(tensor viewed as [n, dim], n, row stride in floats)."""
        if t.dtype != torch.float32 or t.device != self._device or t.dim() < 1 or t.shape[-1] != self.dim:
            raise AssertionError(f"normalize: {what} must be a float32 tensor [..., {self.dim}] on {self._device}")
        if t.dim() == 2 and t.shape[0] > 1 and t.stride(1) == 1 and t.stride(0) >= self.dim:
            return t, int(t.shape[0]), int(t.stride(0))                # rows inside a wider tensor
        if t.dim() == 2 and t.shape[0] == 1 and t.stride(1) == 1:
            return t, 1, self.dim                                       # one row: its stride is never used
        if not t.is_contiguous():
            raise AssertionError(f"normalize: {what} must be contiguous, or two-dimensional with unit column stride")
        t2 = t.view(-1, self.dim)
        return t2, int(t2.shape[0]), self.dim

    def _up(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1, self.dim)).to(self._device)

    # ------------------------------------------------------------------ the two operations
    def update(self, rows, mask=None):
        """Count `rows` ([n, dim]); `mask` (uint8 or bool [n]): only the rows whose byte is non-zero.  A selected row with a non-finite
        value is left out and adds 1 to ``skipped``."""
        if not isinstance(rows, torch.Tensor):
            rows = self._up(rows)
            mask = None if mask is None else torch.from_numpy(np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, dtype=np.uint8)).to(self._device)
        t, n, stride = self._rows(rows, "rows")
        if mask is not None:
            mask = mask.reshape(-1)
            if mask.dtype == torch.bool:
                mask = mask.to(torch.uint8)
            if mask.dtype != torch.uint8 or mask.shape[0] != n or mask.device != self._device or not mask.is_contiguous():
                raise AssertionError(f"normalize: mask must be a contiguous uint8 or bool tensor [{n}] on {self._device}")
        self._after_torch()
        self._norm.update_dev(t.data_ptr(), stride, None if mask is None else mask.data_ptr(), n)
        self._before_torch()

    def apply(self, rows, out=None):
        """clamp((rows - mean32) rstd32, -clip, clip) into `out` (None: a new tensor; `rows` itself: in place) and return it.  Host rows
        give a host array: `out`, a float32 numpy array of their shape, if given."""
        if not isinstance(rows, torch.Tensor):
            host = self.apply(self._up(rows)).cpu().numpy().reshape(np.shape(rows))
            if out is None:
                return host
            if not isinstance(out, np.ndarray) or out.dtype != np.float32 or out.shape != host.shape:
                raise AssertionError("normalize: out for host rows must be a float32 numpy array of their shape")
            out[...] = host
            return out
        if out is None:
            out = torch.empty(rows.shape, dtype=torch.float32, device=self._device)
        if out.shape != rows.shape:
            raise AssertionError("normalize: out must have the shape of rows")
        t, n, stride = self._rows(rows, "rows")
        o, _, ostride = self._rows(out, "out")
        self._after_torch()
        self._norm.apply_dev(t.data_ptr(), stride, o.data_ptr(), ostride, n)
        self._before_torch()
        return out

    # ------------------------------------------------------------------ the statistics
    def state(self):
        """(count, mean [dim], m2 [dim], skipped): the fp64 state as the device keeps it; synchronises."""
        return self._norm.state()

    @property
    def count(self) -> float:
        return self._norm.state()[0]

    @property
    def skipped(self) -> int:
        return self._norm.state()[3]

    @property
    def mean(self):
        return self._norm.state()[1]

    @property
    def std(self):
        """sqrt(max(m2 / count, eps^2)) in fp64 (ones before the first row): what ``published()`` holds the reciprocal of."""
        count, _, m2, _ = self._norm.state()
        return np.sqrt(np.maximum(m2 / count, self.eps ** 2)) if count > 0 else np.ones(self.dim)

    def published(self):
        """(mean32 [dim], rstd32 [dim]): copies of the float32 vectors apply reads, as device tensors."""
        if self._published is None:
            self._published = zero_tensors(self._device, dict(mean32=((self.dim,), torch.float32), rstd32=((self.dim,), torch.float32)))
        p = self._published
        self._after_torch()
        self._norm.published_dev(p["mean32"].data_ptr(), p["rstd32"].data_ptr())
        self._before_torch()
        return p["mean32"], p["rstd32"]

    def state_dict(self) -> dict:
        """Host fp64 arrays; ``load_state_dict`` of it into a RunningNorm of the same dim continues bit for bit."""
        count, mean, m2, skipped = self._norm.state()
        return dict(dim=self.dim, eps=self.eps, clip=self.clip, count=count, mean=mean, m2=m2, skipped=skipped)

    def load_state_dict(self, state: dict):
        if int(state.get("dim", self.dim)) != self.dim:
            raise ValueError(f"load_state_dict: the state has {state['dim']} columns, this normaliser {self.dim}")
        self._norm.set_state(state["count"], state["mean"], state["m2"], state.get("skipped", 0))

    @staticmethod
    def merge_states(states) -> dict:
        """Chan's rule on the host, in list order: the state of the rows of all `states` together.  A sharded run combines its ranks'
        statistics reproducibly by merging them in rank order."""
        states = list(states)
        if not states:
            raise ValueError("merge_states of nothing")
        first = states[0]
        count, mean, m2 = float(first["count"]), np.array(first["mean"], dtype=np.float64), np.array(first["m2"], dtype=np.float64)
        skipped = int(first.get("skipped", 0))
        for s in states[1:]:
            m, mean_b, m2_b = float(s["count"]), np.asarray(s["mean"], dtype=np.float64), np.asarray(s["m2"], dtype=np.float64)
            if mean_b.shape != mean.shape:
                raise ValueError("merge_states: the states differ in their number of columns")
            skipped += int(s.get("skipped", 0))
            if not m > 0.0:
                continue
            delta, tot = mean_b - mean, count + m
            mean = mean + delta * m / tot
            m2 = m2 + (m2_b + delta * delta * count * m / tot)
            count = tot
        return {**{k: first[k] for k in ("dim", "eps", "clip") if k in first}, "count": count, "mean": mean, "m2": m2, "skipped": skipped}

    def clear(self):
        self._norm.clear()

    @property
    def stream(self):
        """The batch's stream as a torch stream: where every call of this object runs."""
        return self._stream

    def close(self):
        self._norm.close()
        self._published = None


class ObsNormalizer:
    """``obs``: a RunningNorm of the env's observation rows; ``goal``: one of 3-float goals.  ``VecHSREnv.make_normalizer`` attaches it to
    the device loop, which then counts every observation the env hands to the policy exactly once and leaves those rows, normalised with
    the statistics that include them, in ``policy_obs`` [n_envs, obs_dim] on the device.  The goal statistics come from relabelled samples
    (the baselines' rule): ``update_goals(batch)``.  ``apply_batch(batch)`` normalises a sampled batch in place, in one launch.

    The statistics are learner state, not env state: ``VecHSREnv.load_state`` and ``fork`` do not change them (keep and restore them with
    ``state_dict`` / ``load_state_dict``)."""

    OBS_KEYS, GOAL_KEYS = ("obs", "next_obs", "nstep_obs"), ("goal", "achieved_next")

    def __init__(self, sim: BatchSim, obs_dim: int, eps: float = 0.01, clip: float = 5.0):
        self.sim = sim
        self.obs, self.goal = RunningNorm(sim, obs_dim, eps, clip), RunningNorm(sim, 3, eps, clip)
        self.policy_obs = zero_tensors(self.obs._device, dict(p=((sim.n, int(obs_dim)), torch.float32)))["p"]

    def observe(self, rows, mask=None):
        """The device loop's hook: count `rows` [n_envs, obs_dim] (those of `mask`), then normalise all of them into ``policy_obs``."""
        self.obs.update(rows, mask)
        self.obs.apply(rows, out=self.policy_obs)

    def update_goals(self, batch):
        """Count ``batch['goal']`` of a sampled (relabelled) batch."""
        self.goal.update(batch["goal"])

    def apply_batch(self, batch):
        """Normalise a batch of ``HindsightReplay.sample`` or ``sample_sequences`` in place, on the replay's stream, in one launch: obs,
        next_obs and nstep_obs with the obs statistics, goal and achieved_next with the goal statistics.  Rows of a window past its
        ``length`` are padding and stay zero."""
        items = []
        for keys, which, norm in ((self.OBS_KEYS, 0, self.obs), (self.GOAL_KEYS, 1, self.goal)):
            for k in keys:
                t = batch.get(k)
                if t is None:
                    continue
                if t.dtype != torch.float32 or not t.is_contiguous() or t.shape[-1] != norm.dim or t.device != norm._device:
                    raise AssertionError(f"normalize: batch[{k!r}] must be a contiguous float32 tensor [..., {norm.dim}] on {norm._device}")
                items.append((t.data_ptr(), t.numel() // norm.dim, t.shape[1] if t.dim() == 3 else 1, which))
        if not items:
            return batch
        length = batch.get("length")
        self.obs._after_torch()
        norm_apply_batch_dev(self.obs._norm, self.goal._norm, items, None if length is None else length.data_ptr())
        self.obs._before_torch()
        return batch

    def state_dict(self) -> dict:
        return dict(obs=self.obs.state_dict(), goal=self.goal.state_dict())

    def load_state_dict(self, state: dict):
        self.obs.load_state_dict(state["obs"])
        self.goal.load_state_dict(state["goal"])

    def close(self):
        self.obs.close()
        self.goal.close()


__all__ = ["RunningNorm", "ObsNormalizer"]
