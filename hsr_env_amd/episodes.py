"""Episodes on the device: the spec ``BatchSim.set_episodes`` uploads (include/hsrsim.h: hsr_episode_spec).

``ResetPlan.from_env`` is the one parse of the arguments of ``VecHSREnv`` - ``starts``, the goals, ``block_space`` - into what a reset
samples and what a step tests: a joint in ``starts`` is sampled over its qpos slice, every other qpos entry keeps ``qpos0``, with
``block_space`` block b occupies ``qpos[nu + 7 b : nu + 7 b + 7]``, and at most one goal holds a point.  The host sampler
(``VecHSREnv.new_state`` / ``reset``) reads the plan, and ``EpisodeSpec`` turns the same plan into the range tables the device sampler
draws from (lo == hi where nothing is sampled).  The draws themselves (Philox4x32-10, keyed by seed and global env id) are csrc/episode.h.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, List, Optional

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
class ResetPlan:
    """What a reset samples and what a step tests, as addresses and ids of the model.  A parse, not a judge: what the env or the device
    sampler cannot do with a plan (two points, an unbounded Box, ...) is refused by ``VecHSREnv`` and ``EpisodeSpec.from_plan``."""
    starts: List[tuple]                     # (joint, start, end, space): the qpos slices of ``starts``, in the dict's order
    block_qadr: List[int]                   # with block_space: the qpos address of every block's free joint
    block_space: Optional[Box]
    points: List[tuple]                     # (goal index, operand) of every goal operand that is not a body name
    goal_body: int                          # the main term, (goal_body, geofence): the goal between a body and the point
    geofence: float
    extra_terms: List[tuple]                # (body a, body b, distance) of the goals between two bodies
    mocap_body: Optional[int]               # the body that carries the point on the device

    @classmethod
    def from_env(cls, model: Model, starts: Optional[Dict[str, Box]] = None, goals=None, block_space: Optional[Box] = None) -> "ResetPlan":
        slices = []
        for joint, space in (starts or {}).items():
            adr = model.joint_qpos_addr(joint)                      # ValueError for a joint the model does not have
            start, end = adr if isinstance(adr, tuple) else (adr, adr + 1)
            slices.append((joint, start, end, space))
        qadr = [model.nu + 7 * b for b in range((model.nq - model.nu) // 7)] if block_space is not None else []
        plan = cls(starts=slices, block_qadr=qadr, block_space=block_space, points=[], goal_body=-1, geofence=0.0, extra_terms=[],
                   mocap_body=next((i for i, mc in enumerate(model.arrays["body_mocap"]) if mc), None))
        for gi, (a, b, d) in enumerate(goals or []):
            bodies = [x for x in (a, b) if isinstance(x, str)]
            plan.points += [(gi, x) for x in (a, b) if not isinstance(x, str)]
            if len(bodies) == 2:
                plan.extra_terms.append((model.body_id(a), model.body_id(b), float(d)))
            elif len(bodies) == 1 and plan.goal_body < 0:
                plan.goal_body, plan.geofence = model.body_id(bodies[0]), float(d)
        return plan

    @property
    def point_goal(self) -> Optional[int]:
        """Which goal holds the point operand."""
        return self.points[0][0] if self.points else None

    @property
    def point(self):
        """The point operand: an array, or a Space to sample."""
        return self.points[0][1] if self.points else None


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
        return cls.from_plan(model, ResetPlan.from_env(model, starts, goals, block_space), seed, env_offset, max_episode_steps)

    @classmethod
    def from_plan(cls, model: Model, plan: "ResetPlan", seed: int = 0, env_offset: int = 0,
                  max_episode_steps: Optional[int] = None) -> "EpisodeSpec":
        qlo = np.asarray(model.qpos0, np.float32).copy()
        qhi = qlo.copy()
        for joint, start, end, space in plan.starts:
            lo, hi = _bounded(space, f"starts[{joint!r}]")
            if lo.size != end - start:
                raise ValueError(f"starts[{joint!r}]: a Box of {lo.size} values for a qpos slice of {end - start}")
            qlo[start:end], qhi[start:end] = lo, hi
        spec = cls(seed=int(seed) & (2 ** 64 - 1), env_offset=int(env_offset), max_episode_steps=int(max_episode_steps or 0),
                   qpos_lo=qlo, qpos_hi=qhi)
        if plan.block_space is not None:
            lo, hi = _bounded(plan.block_space, "block_space")
            if lo.size != 4:
                raise ValueError("block_space is a Box(4): x, y, z, yaw")
            spec.block_qadr = np.array(plan.block_qadr, np.int32)
            spec.block_lo, spec.block_hi = lo, hi
        if len(plan.points) > 1:
            raise ValueError("the goals hold more than one point operand: mocap_pos has room for one")
        if plan.points:
            pt = plan.point
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
