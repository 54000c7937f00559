"""Vectorised counterpart of ``hsr.env.HSREnv`` / ``hsr.mujoco_env.MujocoEnv`` (reference:
hsr/env.py:23-209, hsr/mujoco_env.py:20-151): same constructor arguments, ``step / reset / seed /
set_state``, spaces, goal-within-geofence reward with per-substep early exit - for N envs advanced in
lockstep by libhsrsim (``BatchSim``).  With ``n_envs == 1`` every return value has the reference's scalar
shapes, so the driver loop of hsr/control.py:66-76 runs against it unchanged.

Semantics recorded in SURVEY.md section 8(a) "known reference defects": a goal is
``GoalSpec(a=<body name>, b=<point or Box(3)>, distance)``: success = |xpos(a) - b| < distance with b
written to ``mocap_pos`` at reset (the working shape of hsr/__init__.py:12); ``starts`` maps a joint name
to a Box over its qpos slice, sampled per env at reset (hsr/env.py:149-156).
"""
from __future__ import annotations

from collections import namedtuple
from pathlib import Path
from typing import Dict, List, Optional

import numpy as np

from .episodes import EpisodeSpec, ResetPlan
from .model import Model, load_config
from .sim import raise_if_diverged
from .spaces import Box, Space

GoalSpec = namedtuple("GoalSpec", "a b distance")     # hsr/env.py:20
# what VecHSREnv.save_state returns: the device records of every env (sim.Snapshot) and the host books that belong to them
EnvState = namedtuple("EnvState", "snapshot time_steps goal_points reset_count action_step last_obs began")


def distance_between(pos1, pos2):                        # hsr/env.py:231-232
    return np.sqrt(np.sum(np.square(pos1 - pos2), axis=-1))


def block_space_to_qpos(sample4: np.ndarray) -> np.ndarray:
    """(x, y, z, yaw) of a block -> free-joint qpos (x y z qw qx qy qz); the build's reading of
    ``--block-space`` (a Box(4), hsr/util.py:33), see SURVEY.md section 8(a) defects."""
    s = np.asarray(sample4, dtype=np.float64)
    out = np.zeros(s.shape[:-1] + (7,))
    out[..., :3] = s[..., :3]
    out[..., 3] = np.cos(s[..., 3] / 2)
    out[..., 6] = np.sin(s[..., 3] / 2)
    return out


class VecHSREnv:
    metadata = {"render.modes": "rgb_array"}

    def __init__(self, xml_file=None, goals: Optional[List[GoalSpec]] = None, starts: Optional[Dict[str, Box]] = None,
                 steps_per_action: int = 300, obs_type: str = None, render: bool = False, record: bool = False,
                 record_freq: int = None, render_freq: int = None, record_path: Path = None,
                 n_envs: int = 1, model: Optional[Model] = None, sim=None, device: int = 0,
                 env_offset: int = 0, n_global: Optional[int] = None, block_space: Optional[Box] = None,
                 record_envs: Optional[List[int]] = None, record_size=None, record_camera=None,
                 auto_reset: bool = False, max_episode_steps: Optional[int] = None):
        if model is None:
            model = load_config(str(xml_file)) if xml_file is not None else None
        if model is None:
            raise IOError("File %s does not exist" % xml_file)          # hsr/mujoco_env.py:30-31
        if any([render, render_freq]):
            raise NotImplementedError("render=True / render_freq: the 'human' viewer needs a display (record=True writes videos)")
        if obs_type not in (None, "openai"):
            raise ValueError(f"unknown obs_type {obs_type!r}")
        if obs_type == "openai" and not ({"hand_l_proximal_joint", "hand_r_proximal_joint"} <= set(model.names["joint"]) and model.block_body()):
            raise ValueError("obs_type='openai' needs the two finger joints among the DOFs and a block (hsr/env.py:58-59,90-97)")
        self.model = model
        self.n_envs = int(n_envs)
        self.env_offset, self.n_global = int(env_offset), int(n_global or n_envs)
        self.starts = dict(starts or {})
        self.block_space = block_space
        self.goals_specs = goals
        self.goals = None
        self._time_steps = np.zeros(self.n_envs, dtype=np.int64)
        self._obs_type = obs_type
        self.reward_range = -np.inf, np.inf
        self.spec = None
        self.steps_per_action = steps_per_action
        self.record_freq = record_freq or 20
        self.render_freq = render_freq or 20
        self.frame_skip = self.record_freq                              # hsr/env.py:68 passes record_freq
        # hsr/env.py:58 hard-codes 'block0' (the util.py:109 injection); cupboard-world.xml:113 names its body 'block'
        self._block_name = model.block_body() or "block0"
        self._finger_names = ["hand_l_distal_link", "hand_r_distal_link"]
        if sim is None:
            if auto_reset:
                import torch  # noqa: F401  the device loop's buffers are torch tensors, and torch's HIP runtime must be the first one
                #                            loaded into the process: after the library's, torch finds no GPU
            from .sim import BatchSim
            sim = BatchSim(model, self.n_envs, device=device)
        self.sim = sim
        # episodes on the device (episodes.py, csrc/episode.h): reset states, goals and the time limit are drawn and kept by the batch,
        # and step() resets the envs that finished.  Opt-in; the host-sampled reset below stays what it is.  No CPU stand-in.
        self.auto_reset = bool(auto_reset)
        self.max_episode_steps = int(max_episode_steps or 0)
        if max_episode_steps is not None and not self.auto_reset:
            raise ValueError("max_episode_steps belongs to auto_reset=True (rl.TimeLimit wraps an env without it)")
        if self.auto_reset and not hasattr(sim, "set_episodes"):
            raise NotImplementedError("auto_reset=True needs a simulator handle with set_episodes (BatchSim): episodes run on the device")
        # hsr/env.py:50-66: record when any of record / record_path / record_freq is given.  One video per recorded env (global ids
        # record_envs, default [0]; a rank records the ones in its shard) under the directory record_path (record.py)
        self._recorder = None
        if any([record, record_path, record_freq]):
            from .record import EnvRecorder
            from .render import DEFAULT_SIZE, default_camera
            gids = [int(g) for g in (record_envs if record_envs is not None else [0])]
            if len(set(gids)) != len(gids) or any(g < 0 or g >= self.n_global for g in gids):
                raise ValueError(f"record_envs must be distinct env ids in 0..{self.n_global - 1}")
            mine = [g for g in gids if self.env_offset <= g < self.env_offset + self.n_envs]
            self._recorder = EnvRecorder(sim, Path(record_path or "/tmp/training-video"), mine, [g - self.env_offset for g in mine],
                                         self.record_freq, record_size or DEFAULT_SIZE,
                                         record_camera if record_camera is not None else default_camera(model))
        bounds = model.act_ctrlrange.copy()
        self.action_space = Box(low=bounds[:, 0], high=bounds[:, 1], dtype=np.float32)
        self.init_qpos = model.qpos0.copy()
        self.init_qvel = np.zeros(model.nv)
        self.obs_dim = 25 if obs_type == "openai" else model.nq + model.nv
        high = np.inf * np.ones(self.obs_dim)
        self.observation_space = Box(-high, high, dtype=np.float32)
        self._loop = None              # device_loop.DeviceLoop: the torch side of auto_reset=True, which alone has one
        if self.auto_reset:
            from .device_loop import DeviceLoop
            self._loop = DeviceLoop(sim, self.n_envs, model.nu, model.nq + model.nv, self.obs_dim, openai=obs_type == "openai")
        self._goal_points = np.zeros((self.n_envs, 3), dtype=np.float32)
        self._plan = ResetPlan.from_env(model, self.starts, goals, block_space)      # what a reset samples and a step tests, parsed once
        self._parse_goals()
        self.seed()
        t, q, v = self.sim.get_state()
        self.initial_state = (t.copy(), q.copy(), v.copy())
        self._last_obs = np.concatenate([q, v], axis=1)

    # ------------------------------------------------------------------ helpers
    def _squeeze(self, x):
        return x[0] if self.n_envs == 1 else x

    def _scalar(self, x):
        """A per-env value that the reference holds as a Python scalar."""
        return x[0].item() if self.n_envs == 1 else x

    def _count_step(self, done):
        """Every env has taken one more step -> the success that is logged (hsr/env.py:133)."""
        self._time_steps += 1
        return done & (self._time_steps > 0)

    def _step_result(self, obs, rew, done, success, ns, **episode_info):
        """What step() returns; with n_envs == 1 in the reference's scalar shapes."""
        self._last_obs = obs
        info = {"log count": {"success": self._squeeze(success)}, "substeps": self._squeeze(ns), **episode_info}
        return self._squeeze(obs), self._scalar(rew), self._scalar(done), info

    def _mask(self, mask):
        return np.ones(self.n_envs, dtype=bool) if mask is None else np.asarray(mask, dtype=bool).reshape(self.n_envs)

    def _parse_goals(self):
        """hsr/env.py:124-126,137-147: `done = all(in_range(a, b, d) for a, b, d in goals)`, an operand being a body name
        (its xpos), a point (ndarray, or a Space sampled at reset) or a callable.  On the device a goal is a pair of bodies, or a
        body and THE point: like the reference, whose reset writes the concatenation of all point operands into the single
        mocap_pos[1, 3] (hsr/env.py:169-172), at most one point operand can exist across the goals.  The goal that holds the
        point is the main term of hsr_batch_step (goal_body, geofence); body-body goals become the extra terms of
        hsr_batch_set_goals (the mocap body stands for the point there).  Callables cannot run inside the substep loop.
        The parse is episodes.ResetPlan; what this env refuses of it is here."""
        for a, b, d in self.goals_specs or []:
            for x in (a, b):
                if callable(x) and not isinstance(x, Space):
                    raise RuntimeError(f"{x} must be np.ndarray or string: callables cannot be evaluated inside the device substep loop")
                if not isinstance(x, (str, np.ndarray, Space, list, tuple)):
                    raise RuntimeError(f"{x} must be function, np.ndarray, or string")      # hsr/env.py:145
            if not (isinstance(a, str) or isinstance(b, str)):
                raise RuntimeError("a goal between two points does not depend on the simulation")
        if len(self._plan.points) > 1:
            raise ValueError("the goals hold more than one point operand: mocap_pos has room for one (hsr/env.py:169-172)")
        if len(self._plan.extra_terms) > 4:
            raise NotImplementedError("at most four body-body goals besides the point goal")
        if self._plan.extra_terms and not hasattr(self.sim, "set_goals"):
            raise NotImplementedError("this simulator handle does not evaluate body-body goals")

    @property
    def dt(self):
        return self.model.timestep * self.frame_skip                   # hsr/mujoco_env.py:96-98

    def seed(self, seed=None):
        self._seed = 0 if seed is None else int(seed)
        self._reset_count = 0
        self.np_random = np.random.Generator(np.random.Philox(key=self._seed))
        if self._loop is not None:                                      # the device sampler restarts: same seed, same run
            self._loop.restart(EpisodeSpec.from_plan(self.model, self._plan, seed=self._seed, env_offset=self.env_offset,
                                                     max_episode_steps=self.max_episode_steps))
        return [seed]

    def _global_rng(self):
        # one stream per (seed, reset index); every rank draws the global batch and keeps its shard, so a
        # sharded run reproduces the single-GPU run env for env
        return np.random.Generator(np.random.Philox(key=[self._seed, self._reset_count]))

    def _shard(self, x):
        return x[self.env_offset:self.env_offset + self.n_envs]

    # ------------------------------------------------------------------ gym surface
    def new_state(self, rng=None):
        """hsr/env.py:149-156: qpos with every joint in ``starts`` resampled (per env)."""
        rng = rng or self._global_rng()
        qpos = np.tile(self.model.qpos0, (self.n_global, 1))
        for joint, start, end, space in self._plan.starts:
            assert isinstance(space, Space)
            qpos[:, start:end] = space.sample(self.n_global, rng=rng)
        for a in self._plan.block_qadr:
            qpos[:, a:a + 7] = block_space_to_qpos(self._plan.block_space.sample(self.n_global, rng=rng))
        return self._shard(qpos)

    def _sample_goal_points(self, m, rng):
        """The host sampler's goal point for the envs `m`; the first draws of a reset's stream, before new_state()."""
        pt = self._plan.point
        if pt is None:
            return
        pts = pt.sample(self.n_global, rng=rng) if isinstance(pt, Space) else np.tile(np.asarray(pt, dtype=np.float32), (self.n_global, 1))
        pts = self._shard(np.asarray(pts, dtype=np.float32).reshape(self.n_global, 3))
        self._goal_points[m] = pts[m]

    def _begin_episodes(self, m):
        """The envs `m` start an episode: the recorder closes theirs and their step count restarts."""
        if self._recorder is not None:
            self._recorder.on_reset(m, self._time_steps > 0)
        self._time_steps[m] = 0

    def _begin_goals(self):
        """From the first reset() on the goals are tested (before it `goals is None`: hsr/env.py:39,125)."""
        if self.goals_specs and self.goals is None:
            if self._plan.extra_terms:
                self.sim.set_goals(self._plan.extra_terms)
            self.goals = list(self.goals_specs)

    def _refresh_goal_points(self):
        """The goal points the device drew (its mocap_pos) -> ``goals`` / ``in_range``."""
        if self._plan.point_goal is not None and self.goals is not None:
            self._goal_points = np.asarray(self.sim.body_xpos(self._plan.mocap_body), dtype=np.float32)
            self._publish_goal_points()

    def _publish_goal_points(self):
        """``goals`` holds the point goal with the current ``_goal_points``."""
        gi = self._plan.point_goal
        if gi is None or self.goals is None:
            return
        a, b, d = self.goals_specs[gi]
        cur = self._squeeze(self._goal_points)
        self.goals[gi] = GoalSpec(a, cur, d) if isinstance(a, str) else GoalSpec(cur, b, d)

    def reset(self, mask=None):
        """sim.reset() + reset_model() (hsr/mujoco_env.py:83-85, hsr/env.py:158-177); ``mask`` selects envs.  With auto_reset=True the
        device draws the episodes (and the goal points this object then reads back)."""
        m = self._mask(mask)
        self._begin_episodes(m)
        self._begin_goals()
        if self._loop is not None:
            self._loop.reset(m)
            self._refresh_goal_points()
            obs = self._get_observation()
            self._loop.commit_host_rows(self._last_obs, m)
            return obs
        rng = self._global_rng()
        self._reset_count += 1
        self._sample_goal_points(m, rng)
        self._publish_goal_points()
        qpos = self.new_state(rng).astype(np.float32)
        self.sim.reset(mask=m.astype(np.uint8), qpos0=qpos, mocap=self._goal_points)
        return self._get_observation()

    def sample_action_dev(self):
        """Uniform actions over the action space drawn on the device (torch float32 [n_envs, nu]); every call is the next action step."""
        return self._loop.sample_action()

    # ------------------------------------------------------------------ hindsight replay on the device (replay.py)
    def make_replay(self, capacity_steps: int, her_ratio: float = 0.8, seed: Optional[int] = None, prioritized: bool = False, alpha: float = 0.6,
                    eps: float = 1e-6, **priority_options):
        """Attach a replay.HindsightReplay to the device loop and return it: from now on every step() records its transition (between the
        step and the episode end, so the achieved goal is the one of the step, not of the next episode's start) and commits the
        observation it returns, and reset() commits too; ``replay.sample(batch_size)`` then draws relabelled minibatches without a copy
        to the host, and ``replay.sample_sequences(batch_size, seq_len, gamma)`` windows of up to seq_len steps inside one episode with
        their n-step targets.  Rows are this env's observations (25 floats with obs_type='openai').  seed None: the env's seed.
        prioritized=True: samples are drawn by priority (|td| + eps)^alpha and carry importance weights; feed the learner's TD errors back
        with ``replay.update_priorities(batch, td_error)`` (priority_options: p_max, max_batch of replay.HindsightReplay)."""
        if self._loop is None:
            raise ValueError("make_replay needs auto_reset=True: the replay is fed by the device loop, which only that mode runs")
        if self._plan.point_goal is None:
            raise NotImplementedError("make_replay needs a point goal (a body and a point): hindsight relabelling replaces that point by a "
                                      "position the body reached")
        if self._plan.extra_terms:
            raise NotImplementedError("make_replay with body-body goals besides the point goal: their reward cannot be recomputed from a relabelled point")
        if self._loop.replay is not None:
            raise ValueError("this env already feeds a replay")
        from .replay import HindsightReplay
        replay = HindsightReplay(self.sim, capacity_steps, self._plan.goal_body, self._plan.geofence, obs_dim=self.obs_dim, her_ratio=her_ratio,
                                 seed=self._seed if seed is None else seed, env_offset=self.env_offset, prioritized=prioritized, alpha=alpha, eps=eps,
                                 **priority_options)
        self._loop.attach_replay(replay)
        self._get_observation()
        # (a rollout begins again too: the loop's tensors were made anew.)  Not counted by a normaliser: the policy had these rows before
        self._loop.commit_host_rows(self._last_obs, count=False)
        return replay

    # ------------------------------------------------------------------ on-policy rollouts on the device (rollout.py)
    def make_rollout(self, horizon: int, gamma: float = 0.99, lam: float = 0.95, seed: Optional[int] = None):
        """Attach a rollout.OnPolicyRollout of `horizon` env-steps to the device loop and return it: ``rollout.obs`` is what the policy acts
        on, ``rollout.stage(action, logp, value)`` must precede every step(), which then closes the step with its reward, its reset kind and
        the rows it returns; ``rollout.terminal_obs`` holds info['terminal_observation'] on the device for the critic's
        ``rollout.bootstrap(...)``.  After `horizon` steps: ``finish``, ``minibatches``, ``next``.  reset(), load_state() and fork() start
        the rollout again from the current rows.  Rows are this env's observations (25 floats with obs_type='openai').  seed None: the
        env's seed; env_offset is passed on, so a shard draws its own shuffle."""
        if self._loop is None:
            raise ValueError("make_rollout needs auto_reset=True: the rollout is fed by the device loop, which only that mode runs")
        if self._loop.rollout is not None:
            raise ValueError("this env already feeds a rollout")
        from .rollout import OnPolicyRollout
        rollout = OnPolicyRollout(self.sim, horizon, obs_dim=self.obs_dim, gamma=gamma, lam=lam, seed=self._seed if seed is None else seed,
                                  env_offset=self.env_offset)
        self._loop.attach_rollout(rollout)
        self._get_observation()
        self._loop.begin_rollout(self._last_obs)
        return rollout

    # ------------------------------------------------------------------ observation and goal normalisation on the device (normalize.py)
    def make_normalizer(self, eps: float = 0.01, clip: float = 5.0):
        """Attach a normalize.ObsNormalizer to the device loop and return it: running fp64 mean / std of the observation columns
        (``normalizer.obs``) and of the 3-float goal (``normalizer.goal``) on the device.  Every observation the env hands to the policy
        is counted exactly once: the current rows of all envs now, the rows of the envs a reset() resets, the rows every step() returns (as
        the last link of the step, after the replay's commit and the rollout's close).  After each of them ``normalizer.policy_obs``
        [n_envs, obs_dim] holds the normalised rows on the device for a policy to read without a copy.  What step() and reset() return,
        and what a replay or rollout stores, stays raw: statistics move, so stored rows are normalised when they are read
        (``replay.sample(..., normalizer=normalizer)``, ``normalizer.apply_batch``).  Goal statistics come from relabelled samples:
        ``normalizer.update_goals(batch)``.
        load_state() and fork() do not change the statistics: they are learner state, not env state (keep them with
        ``normalizer.state_dict()``); policy_obs follows the rows they jump to."""
        if self._loop is None:
            raise ValueError("make_normalizer needs auto_reset=True: the normaliser is fed by the device loop, which only that mode runs")
        if self._loop.normalizer is not None:
            raise ValueError("this env already feeds a normaliser")
        from .normalize import ObsNormalizer
        normalizer = ObsNormalizer(self.sim, self.obs_dim, eps=eps, clip=clip)
        self._loop.attach_normalizer(normalizer)
        self._get_observation()
        self._loop.observe_host_rows(self._last_obs)
        return normalizer

    # ------------------------------------------------------------------ planning on the device (planner.py)
    def make_planner(self, samples: int = 64, horizon: int = 3, **options):
        """A planner.CEMPlanner for this env: ``planner.plan()`` returns the action to take now in every env, a torch tensor on the device
        that step() takes as it is with auto_reset=True (``.cpu().numpy()`` without).  It forks every env `samples` times into a batch of
        its own, plays sampled action sequences of `horizon` env-steps there and refits; this env is only read, through a snapshot, and
        behaves bit for bit as without a planner.  Nothing is attached to the env: call ``plan()`` when an action is wanted, with
        ``fresh=`` the envs whose episode just began.  options: iterations, elites, gamma, alpha, init_std, min_std, seed (None: the
        env's) of planner.CEMPlanner; a shard passes its env_offset on.  Needs a goal with a body and a point (ValueError otherwise) and a
        simulator handle with snapshots (BatchSim)."""
        if not hasattr(self.sim, "snapshot"):
            raise NotImplementedError("make_planner needs a simulator handle with snapshots (BatchSim): the candidates are exact forks")
        from .planner import CEMPlanner
        return CEMPlanner(self, samples, horizon, **options)

    # ------------------------------------------------------------------ exact snapshots (sim.Snapshot)
    def _no_jump_while_recording(self, what):
        if self._recorder is not None:
            raise NotImplementedError(f"{what} while a recorder is attached: a video cannot jump")

    def save_state(self) -> EnvState:
        """sim.get_state() in its exact form (hsr/env.py:69,150; hsr/mujoco_env.py:87-94): every env's device record - state, warm start,
        collision caches, poses, episode books - and this object's own books.  load_state() of it continues bit for bit."""
        self._no_jump_while_recording("save_state")
        snap = self.sim.snapshot()
        snap.save()
        return EnvState(snap, self._time_steps.copy(), self._goal_points.copy(), self._reset_count, self._loop.action_step if self._loop is not None else 0,
                        self._last_obs.copy(), self.goals is not None)

    def load_state(self, state: EnvState):
        """sim.set_state() in its exact form (hsr/env.py:175; hsr/mujoco_env.py:87-94): no forward pass, nothing recomputed.  A replay made by
        make_replay() is cleared: a ring of past transitions cannot follow a jump; a rollout made by make_rollout() starts again."""
        self._no_jump_while_recording("load_state")
        if state.began != (self.goals is not None):
            raise ValueError("load_state: the state was saved on the other side of the first reset()")
        state.snapshot.load(into=self.sim)
        self._time_steps[:] = state.time_steps
        self._goal_points = state.goal_points.copy()
        self._reset_count = state.reset_count
        self._last_obs = state.last_obs.copy()
        self._publish_goal_points()
        if self._loop is not None:
            self._loop.action_step = state.action_step
            self._loop.restart_replay(self._last_obs)

    def fork(self, src, dst):
        """Envs `dst` become copies of env(s) `src` (one id for all, or one per destination), on the device, and continue bit for bit as
        their sources do; with auto_reset=True their next episodes are drawn with their own env ids.  A replay made by make_replay() is
        cleared: a ring of past transitions cannot follow a jump; a rollout made by make_rollout() starts again."""
        self._no_jump_while_recording("fork")
        dst = np.atleast_1d(np.asarray(dst, dtype=np.int32))
        src = np.broadcast_to(np.asarray(src, dtype=np.int32), dst.shape).copy()
        self.sim.copy_envs(src, dst)
        self._time_steps[dst] = self._time_steps[src]
        self._goal_points[dst] = self._goal_points[src]
        self._last_obs[dst] = self._last_obs[src]
        self._publish_goal_points()
        if self._loop is not None:
            self._loop.restart_replay(self._last_obs)

    def set_state(self, qpos, qvel):
        qpos = np.asarray(qpos, dtype=np.float32).reshape(self.n_envs, -1)
        qvel = np.asarray(qvel, dtype=np.float32).reshape(self.n_envs, -1)
        assert qpos.shape[1:] == (self.model.nq,) and qvel.shape[1:] == (self.model.nv,)   # hsr/mujoco_env.py:88-89
        t = self.sim.get_state()[0]
        self.sim.set_state(t, qpos, qvel)

    def state_vector(self):
        return self._get_observation()

    def _get_observation(self):
        if self._obs_type == "openai":                                  # hsr/env.py:72-110, fused on the device
            self._last_obs = self.sim.obs_openai()
            return self._squeeze(self._last_obs)
        t, q, v = self.sim.get_state()
        self._last_obs = np.concatenate([q, v], axis=1)                 # hsr/env.py:111-113
        return self._squeeze(self._last_obs)

    def step(self, action, steps=None):
        """hsr/env.py:115-135 for every env: returns (obs, reward, done, info).  With auto_reset=True the envs that are done or out of
        time are reset inside the call: done = done | truncated, info['terminal_observation'] is what the step itself produced,
        info['TimeLimit.truncated'] and info['episode'] = {'r', 'l'} (valid where done) describe the episode that ended, and the
        returned rows of those envs are the first observation of their next episode.  `action` may then be a torch tensor on the device."""
        steps = steps or self.steps_per_action
        goal_body = self._plan.goal_body if self.goals else -1
        openai = self._obs_type == "openai"
        if self._loop is None:
            action = np.asarray(action, dtype=np.float32).reshape(self.n_envs, self.model.nu)
            obs, rew, done, ns = self.sim.step(action, steps, goal_body, self._plan.geofence)
            raise_if_diverged(self.sim)
            success = self._count_step(done)
            if self._recorder is not None:
                self._recorder.after_step(done, ns)
            if openai:
                obs = self.sim.obs_openai()
            return self._step_result(obs, rew, done, success, ns)
        r = self._loop.step(action, steps, goal_body, self._plan.geofence, openai, self._recorder)
        success = self._count_step(r.done.astype(bool))
        reset = r.kind != 0
        self._begin_episodes(reset)
        if reset.any():
            self._refresh_goal_points()
        obs = r.obs
        if openai:                                                      # no env was reset: the rows read before the episode end still hold
            obs = self.sim.obs_openai() if reset.any() else r.terminal_obs
        return self._step_result(obs, r.reward, reset, success, r.nsteps, **{
            "terminal_observation": self._squeeze(r.terminal_obs), "TimeLimit.truncated": self._scalar(r.kind == 2),
            "episode": {"r": self._scalar(r.fin_return), "l": self._scalar(r.fin_length)}})

    def in_range(self, a, b, distance):
        def parse(x):
            if callable(x):
                return x()
            if isinstance(x, np.ndarray):
                return x
            if isinstance(x, str):
                return self._squeeze(self.sim.body_xpos(self.model.body_id(x)))
            raise RuntimeError(f"{x} must be function, np.ndarray, or string")
        return distance_between(parse(a), parse(b)) < distance

    def block_pos(self):
        return self._squeeze(self.sim.body_xpos(self.model.body_id(self._block_name)))

    def gripper_pos(self):
        f1, f2 = [self.sim.body_xpos(self.model.body_id(n)) for n in self._finger_names]
        return self._squeeze((f1 + f2) / 2.)

    def get_body_com(self, body_name):
        return self._squeeze(self.sim.body_xpos(self.model.body_id(body_name)))

    def render(self, mode="rgb_array", width=500, height=500, camera=None):
        """hsr/mujoco_env.py:105-125 for every env: 'rgb_array' -> uint8 [N,H,W,3], 'depth_array' -> float32 [N,H,W] (distance along
        the camera axis), row 0 at the top; one env's image alone when n_envs == 1.  camera: render.Camera (None: the model's
        default_camera).  A ray caster over the collision geoms (hsr_env_amd/render.py).  'human' needs a display: NotImplementedError."""
        if mode == "rgb_array":
            return self._squeeze(self.sim.render(width, height, camera, rgb=True))
        if mode == "depth_array":
            return self._squeeze(self.sim.render(width, height, camera, rgb=False, depth=True))
        if mode == "human":
            raise NotImplementedError("render('human') needs a display; use 'rgb_array' (python -m hsr_env_amd.render writes images)")
        raise ValueError(f"unknown render mode {mode!r}")

    def close(self):
        if getattr(self, "_recorder", None) is not None:
            self._recorder.close()
        if getattr(self.sim, "close", None):
            self.sim.close()

    def __enter__(self):
        return self

    def __exit__(self, *args):
        self.close()


HSREnv = VecHSREnv
