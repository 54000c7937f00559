"""Planning on the device with the simulator as the model (include/hsrsim.h: hsr_plan; DESIGN.md "Planning on the device").

The reward of this task is sparse (``float(success)``), so a learner starts from nothing; a sampling-based planner is the standard source of
a baseline controller and of demonstrations for the replay.  ``CEMPlanner`` is a cross-entropy-method controller over exact forks of the
acting envs: for each of the P acting envs it keeps a Gaussian over action sequences of H env-steps, copies the env's record into K envs of
a second batch (the *planning batch*, P K envs of the same model on the same device), plays K sampled sequences there, refits the Gaussian
to the E cheapest ones and repeats; the action is the first step of the mean.  Cost of a sequence = the discounted sum of the goal body's
distance to the goal point after each env-step, cut where the step reaches the goal.

The acting batch is only read, once per ``plan()``, through a snapshot: it behaves bit for bit as it would without a planner.  A plan is a
pure function of (seed, env_offset + env, call, acting state): two planners with one seed return the same bits, and a shard plans what the
single batch plans for the same envs.

Plumbing only: draws, costs, rank and refit are the kernels of csrc/plan.h, one launch each between the env-steps of the planning batch;
nothing visits the host inside ``plan()``.  There is no CPU stand-in.  torch must be imported before the first ``BatchSim`` of the process
(its HIP runtime has to be the first one loaded); ``VecHSREnv(auto_reset=True)`` sees to that itself.
"""
from __future__ import annotations

import numpy as np
import torch

from .device_loop import batch_stream
from .sim import BatchSim, PlanSpec


class CEMPlanner:
    """``plan(fresh=None)`` -> torch float32 [n_envs, nu] on the device: the action to take now in every env of `env`.

    samples = K candidates per env, horizon = H env-steps (of ``env.steps_per_action`` substeps), `iterations` refits per call; elites
    (default max(2, K // 8), at most K) candidates refit mean and sigma with step alpha; the cost is discounted with gamma; sigma starts at
    init_std and never falls below min_std, both in units of half an actuator's range.  seed None: the env's seed.  The env needs a goal with
    a body and a point (ValueError otherwise); goals of several terms are refused as the library refuses them."""

    def __init__(self, env, samples: int, horizon: int, iterations: int = 3, elites=None, gamma: float = 1.0, alpha: float = 1.0,
                 init_std: float = 0.5, min_std: float = 0.05, seed=None, env_offset=None):
        plan = env._plan
        if plan.point_goal is None or plan.goal_body is None or plan.goal_body < 0:
            raise ValueError("make_planner needs a goal with a body and a point: the planner's cost is the distance between the two")
        if not 1 <= int(iterations) <= 256:
            raise ValueError("iterations outside 1..256")
        self.env, self.acting = env, env.sim
        self.P, self.K, self.H, self.iterations = int(env.n_envs), int(samples), int(horizon), int(iterations)
        self.goal_body, self.geofence, self.steps = int(plan.goal_body), float(plan.geofence), int(env.steps_per_action)
        self.call = 0
        self.sim = self.cem = self.snapshot = None      # the planning batch, its sim.Plan, the acting envs' records
        # what an env record does not hold: the extra goal terms (the library refuses a planner on a batch that has any)
        self.sim = BatchSim(env.model, self.P * self.K, device=getattr(self.acting, "device", 0))
        try:
            if plan.extra_terms:
                self.sim.set_goals(plan.extra_terms)
            spec = PlanSpec(seed=int(env._seed if seed is None else seed) & (2 ** 64 - 1), env_offset=int(env.env_offset if env_offset is None else env_offset),
                            groups=self.P, samples=self.K, horizon=self.H, elites=int(max(2, self.K // 8) if elites is None else elites),
                            goal_body=self.goal_body, geofence=self.geofence, gamma=gamma, alpha=alpha, init_std=init_std, min_std=min_std)
            self.cem = self.sim.plan(spec)
            self.spec = spec
            # one snapshot for the acting envs' records, slot p = env p.  hsr_batch_snapshot_load_dev bounds the envs of one call by the
            # snapshot's capacity, and a load fills all P K candidates in one launch: capacity P K, of which the slots 0 .. P - 1 are used
            self.snapshot = self.acting.snapshot(self.P * self.K)
            self.device, self.stream = batch_stream(self.sim)
            N, nu = self.P * self.K, env.model.nu
            with torch.cuda.device(self.device):
                self.fan_slot = (torch.arange(N, dtype=torch.int32, device=self.device) // self.K).contiguous()      # the fan-out: candidate e <- slot e // K
                self.fan_env = torch.arange(N, dtype=torch.int32, device=self.device)
                self._ctrl = torch.zeros((N, nu), dtype=torch.float32, device=self.device)
                self._action = torch.zeros((self.P, nu), dtype=torch.float32, device=self.device)
                self._mask = torch.zeros((2, self.P), dtype=torch.uint8, device=self.device)
            torch.cuda.synchronize(self.device)                        # the fills ran on torch's stream, the batch has its own
        except BaseException:
            self.close()
            raise

    def close(self):
        for name in ("cem", "snapshot", "sim"):
            obj = getattr(self, name, None)
            if obj is not None:
                obj.close()
                setattr(self, name, None)

    def __enter__(self):
        return self

    def __exit__(self, *args):
        self.close()

    # ------------------------------------------------------------------ one decision
    def plan(self, fresh=None, mark=None):
        """The action for every acting env now.  `fresh` (bool / uint8 [n_envs], host or device; None: no env): the envs whose episode
        just began - their plan starts again from zero mean and the initial sigma; the others first shift the previous plan by one step.
        The returned tensor is the planner's own and holds until the next call; the planning stream has finished when this returns.
        mark (tools/plan_bench.py): called as mark("planner") / mark("step") after the launches of each kind, inside the planning stream."""
        P, H, plan, sim = self.P, self.H, self.cem, self.sim
        mark = mark or (lambda kind: None)
        ctrl = self._ctrl.data_ptr()
        self.snapshot.save()                                            # the acting envs' records; waits for the acting stream, once
        with torch.cuda.stream(self.stream):
            if fresh is not None:
                f = fresh if isinstance(fresh, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(fresh).reshape(P) != 0))
                f = f.to(self.device).reshape(P) != 0
                self._mask[0].copy_(f)
                self._mask[1].copy_(~f)
            mark("start")
            if self.call > 0:                                           # a new planner is a reset one
                if fresh is None:
                    plan.shift_dev(None)
                else:
                    plan.reset_dev(self._mask[0].data_ptr())
                    plan.shift_dev(self._mask[1].data_ptr())
            elif fresh is not None:
                plan.reset_dev(self._mask[0].data_ptr())
            for it in range(self.iterations):
                self.snapshot.load(self.fan_slot, self.fan_env, into=sim)
                plan.begin_dev()
                for h in range(H):
                    plan.sample_dev(self.call, it, h, ctrl)
                    mark("planner")
                    sim.step_dev(ctrl, self.steps, self.goal_body, self.geofence)
                    mark("step")
                    plan.accumulate_dev(h)
                plan.update_dev()
            plan.action_dev(self._action.data_ptr())
            mark("planner")
            self.stream.synchronize()
        self.call += 1
        return self._action

    # ------------------------------------------------------------------ diagnostics (each waits for the planning stream)
    def _read(self, fn, *shapes_dtypes):
        with torch.cuda.stream(self.stream):
            outs = [torch.zeros(shape, dtype=dt, device=self.device) for shape, dt in shapes_dtypes]
            fn(*[o.data_ptr() for o in outs])
            self.stream.synchronize()
        return [o.cpu().numpy() for o in outs]

    def costs(self):
        """J of every candidate of the last iteration, float32 [n_envs, K]."""
        return self._read(lambda j: self.cem.costs_dev(j, None), ((self.P, self.K), torch.float32))[0]

    def reach_step(self):
        """The horizon step at which every candidate of the last iteration reached the goal, -1 = not: int32 [n_envs, K]."""
        return self._read(lambda r: self.cem.costs_dev(None, r), ((self.P, self.K), torch.int32))[0]

    def best(self):
        """(index int32 [n_envs], cost float32 [n_envs]) of every env's cheapest candidate at the last refit."""
        return tuple(self._read(self.cem.best_dev, ((self.P,), torch.int32), ((self.P,), torch.float32)))

    def state(self):
        """(mean, sigma), float32 [n_envs, H, nu] each."""
        shape = (self.P, self.H, self.env.model.nu)
        return tuple(self._read(self.cem.state_dev, (shape, torch.float32), (shape, torch.float32)))

    @property
    def failed(self):
        """Refits of every env that found no candidate with a finite cost (mean and sigma then stay), uint32 [n_envs]."""
        return self.cem.failed()
