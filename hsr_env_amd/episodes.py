"""Episodes on the device: the spec ``BatchSim.set_episodes`` uploads (include/hsrsim.h: hsr_episode_spec).

``EpisodeSpec.from_env`` turns the arguments of ``VecHSREnv`` - ``starts``, the goals, ``block_space`` - into the range tables the
device sampler draws from, with the joint-address and block-slot rules of ``VecHSREnv.new_state``: a joint in ``starts`` is sampled
over its qpos slice, every other qpos entry keeps ``qpos0`` (lo == hi), and with ``block_space`` block b occupies
``qpos[nu + 7 b : nu + 7 b + 7]``.  The draws themselves (Philox4x32-10, keyed by seed and global env id) are csrc/episode.h.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np

from .model import Model
from .spaces import Box, Space


class CEpisodeSpec(C.Structure):
    """include/hsrsim.h: hsr_episode_spec."""
    _fields_ = [("seed", C.c_uint64), ("env_offset", C.c_uint32), ("max_episode_steps", C.c_int32),
                ("qpos_lo", C.POINTER(C.c_float)), ("qpos_hi", C.POINTER(C.c_float)),
                ("has_goal", C.c_int32), ("goal_lo", C.c_float * 3), ("goal_hi", C.c_float * 3),
                ("nblock", C.c_int32), ("block_qadr", C.POINTER(C.c_int32)),
                ("block_lo", C.c_float * 4), ("block_hi", C.c_float * 4)]


def _bounded(space: Box, what: str):
    if not isinstance(space, Box):
        raise ValueError(f"{what}: the device sampler draws from a Box, got {type(space).__name__}")
    lo, hi = np.asarray(space.low, np.float32).ravel(), np.asarray(space.high, np.float32).ravel()
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        raise ValueError(f"{what}: an unbounded Box cannot be sampled uniformly on the device")
    if np.any(lo > hi):
        raise ValueError(f"{what}: low > high")
    return lo, hi


@dataclass
class EpisodeSpec:
    seed: int
    env_offset: int
    max_episode_steps: int
    qpos_lo: np.ndarray                     # float32 [nq]
    qpos_hi: np.ndarray
    has_goal: bool = False
    goal_lo: np.ndarray = field(default_factory=lambda: np.zeros(3, np.float32))
    goal_hi: np.ndarray = field(default_factory=lambda: np.zeros(3, np.float32))
    block_qadr: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))
    block_lo: np.ndarray = field(default_factory=lambda: np.zeros(4, np.float32))
    block_hi: np.ndarray = field(default_factory=lambda: np.zeros(4, np.float32))

    @classmethod
    def from_env(cls, model: Model, starts: Optional[Dict[str, Box]] = None, goals=None, block_space: Optional[Box] = None,
                 seed: int = 0, env_offset: int = 0, max_episode_steps: Optional[int] = None) -> "EpisodeSpec":
        qlo = np.asarray(model.qpos0, np.float32).copy()
        qhi = qlo.copy()
        for joint, space in (starts or {}).items():
            adr = model.joint_qpos_addr(joint)                      # ValueError for a joint the model does not have
            start, end = adr if isinstance(adr, tuple) else (adr, adr + 1)
            lo, hi = _bounded(space, f"starts[{joint!r}]")
            if lo.size != end - start:
                raise ValueError(f"starts[{joint!r}]: a Box of {lo.size} values for a qpos slice of {end - start}")
            qlo[start:end], qhi[start:end] = lo, hi
        spec = cls(seed=int(seed) & (2 ** 64 - 1), env_offset=int(env_offset), max_episode_steps=int(max_episode_steps or 0),
                   qpos_lo=qlo, qpos_hi=qhi)
        if block_space is not None:
            lo, hi = _bounded(block_space, "block_space")
            if lo.size != 4:
                raise ValueError("block_space is a Box(4): x, y, z, yaw")
            nb = (model.nq - model.nu) // 7
            spec.block_qadr = np.array([model.nu + 7 * b for b in range(nb)], np.int32)
            spec.block_lo, spec.block_hi = lo, hi
        points = [x for g in (goals or []) for x in (g[0], g[1]) if not isinstance(x, str)]
        if len(points) > 1:
            raise ValueError("the goals hold more than one point operand: mocap_pos has room for one")
        if points:
            pt = points[0]
            if isinstance(pt, Space):
                lo, hi = _bounded(pt, "goal space")
            else:
                lo = hi = np.asarray(pt, np.float32).ravel()
                if not np.all(np.isfinite(lo)):
                    raise ValueError("goal point is not finite")
            if lo.size != 3:
                raise ValueError("a goal point has three coordinates")
            spec.has_goal, spec.goal_lo, spec.goal_hi = True, lo.copy(), hi.copy()
        return spec

    def to_c(self):
        """(hsr_episode_spec, the arrays it points into - keep them alive for the call)."""
        qlo = np.ascontiguousarray(self.qpos_lo, np.float32); qhi = np.ascontiguousarray(self.qpos_hi, np.float32)
        qadr = np.ascontiguousarray(self.block_qadr, np.int32)
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        c = CEpisodeSpec(seed=int(self.seed) & (2 ** 64 - 1), env_offset=int(self.env_offset), max_episode_steps=int(self.max_episode_steps),
                         qpos_lo=qlo.ctypes.data_as(fp), qpos_hi=qhi.ctypes.data_as(fp), has_goal=int(bool(self.has_goal)),
                         goal_lo=(C.c_float * 3)(*[float(x) for x in self.goal_lo]), goal_hi=(C.c_float * 3)(*[float(x) for x in self.goal_hi]),
                         nblock=len(qadr), block_qadr=qadr.ctypes.data_as(ip) if len(qadr) else None,
                         block_lo=(C.c_float * 4)(*[float(x) for x in self.block_lo]), block_hi=(C.c_float * 4)(*[float(x) for x in self.block_hi]))
        return c, (qlo, qhi, qadr)
