"""The CEM planner on the device (include/hsrsim.h: hsr_plan; hsr_env_amd/planner.py) against the numpy restatement of tests/plan_ref.py:
draws, costs, rank and refit are the stated functions bit for bit (sigma: one float32 ulp, its fp64 square root being the one rounding
that is not pinned), a plan is reproducible from (seed, env_offset, call), the acting env never notices a planner, and the planner moves
the hand towards a goal.

cfg3, 5 substeps per env-step, `block0` as the goal body with the goal box and geofence of tests/test_gpu_episodes.py, P = 3 groups unless
a test says otherwise."""
import numpy as np
import pytest
import torch        # before the library: torch's HIP runtime must be the first one loaded into the process (as in test_rl.py)

import plan_ref as ref
from hsr_env_amd.env import GoalSpec, VecHSREnv
from hsr_env_amd.sim import BatchSim, PlanSpec
from hsr_env_amd.spaces import Box

pytestmark = pytest.mark.gpu
P, SUB, GEOFENCE, H = 3, 5, 0.05, 3
SEED = 2 ** 40 + 7
BLOCK_START = Box([-.05, -.05, .422, 1, 0, 0, 0], [.05, .05, .422, 1, 0, 0, 0])
GOAL = Box([-.05, -.05, .422], [.05, .05, .422])
MOCAP_BODY = 1
f32 = np.float32
NP_OF = {torch.float32: np.float32, torch.uint8: np.uint8, torch.int32: np.int32}


def u32(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def bits_equal(a, b):
    return np.array_equal(u32(a), u32(b))


def ulps(a, b):
    return np.abs(u32(a).astype(np.int64) - u32(b).astype(np.int64))


class Rig:
    """A planning batch of P K envs of `m`, its planner and the device arrays the planner's calls read and write."""

    def __init__(self, m, K, horizon=H, elites=2, groups=P, gamma=1.0, alpha=1.0, init_std=0.5, min_std=0.05, seed=SEED, env_offset=0, goal_body=None):
        self.m, self.P, self.K, self.H, self.N, self.nu = m, groups, K, horizon, groups * K, m.nu
        self.goal_body = m.body_id("block0") if goal_body is None else goal_body
        self.sim = BatchSim(m, self.N)
        self.spec = PlanSpec(seed=seed, env_offset=env_offset, groups=groups, samples=K, horizon=horizon, elites=elites, goal_body=self.goal_body,
                             geofence=GEOFENCE, gamma=gamma, alpha=alpha, init_std=init_std, min_std=min_std)
        self.plan = self.sim.plan(self.spec)
        dev = torch.device("cuda", 0)
        z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
        self.t = dict(ctrl=z((self.N, self.nu)), J=z(self.N), reach=z(self.N, torch.int32), mean=z((groups, horizon, self.nu)), sigma=z((groups, horizon, self.nu)),
                      extra=z(self.N), mask=z(groups, torch.uint8), best=z(groups, torch.int32), best_cost=z(groups), done=z(self.N, torch.uint8),
                      action=z((groups, self.nu)))
        torch.cuda.synchronize()
        self.lo, self.hi = ref.ctrl_range(m.act_ctrlrange)
        self.half = ref.half_range(self.lo, self.hi)

    def close(self):
        self.plan.close()
        self.sim.close()

    def p(self, k):
        return self.t[k].data_ptr()

    def put(self, k, a):
        self.sim.sync()
        self.t[k].copy_(torch.from_numpy(np.ascontiguousarray(a, NP_OF[self.t[k].dtype]).reshape(tuple(self.t[k].shape))))
        torch.cuda.synchronize()

    def host(self, *keys):
        self.sim.sync()
        return [self.t[k].cpu().numpy() for k in keys]

    def state(self):
        """(mean, sigma, J, reach_step, best index, best cost, failed) as the device holds them."""
        self.plan.state_dev(self.p("mean"), self.p("sigma"))
        self.plan.costs_dev(self.p("J"), self.p("reach"))
        self.plan.best_dev(self.p("best"), self.p("best_cost"))
        return self.host("mean", "sigma", "J", "reach", "best", "best_cost") + [self.plan.failed()]

    def sample(self, call, it, h):
        """-> ctrl float32 [P, K, nu] of step h as the device drew it."""
        self.plan.sample_dev(call, it, h, self.p("ctrl"))
        return self.host("ctrl")[0].reshape(self.P, self.K, self.nu)

    def ref_sample(self, mean, sigma, call, it, h):
        z = ref.z_draws(self.spec.seed, self.spec.env_offset, self.P, self.K, self.H, self.nu, call, it, h)
        return ref.sample(mean, sigma, z, h, self.lo, self.hi)

    def sample_horizon(self, call, it):
        """begin, then every step of the horizon sampled -> the actions as sampled, float32 [P, H, nu, K]."""
        self.plan.begin_dev()
        return np.stack([self.sample(call, it, h) for h in range(self.H)], axis=1).transpose(0, 1, 3, 2).copy()

    def ref_update(self, mean, sigma, act, J, failed):
        out = [ref.update(mean[p], sigma[p], act[p], J[p * self.K:(p + 1) * self.K], self.spec.elites, self.spec.alpha, self.spec.min_std, self.half)
               for p in range(self.P)]
        return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[3] for o in out]), np.array([o[4] for o in out], f32),
                failed + np.array([o[5] for o in out], np.uint32))


def planted_costs(case, rng, n, K, elites):
    """The cost cases of the update test, float32 [n] for groups of K."""
    if case == "distinct":
        return rng.permutation(n).astype(f32) * f32(0.37) - f32(3)
    if case == "equal":
        return np.full(n, 1.25, f32)
    if case == "some_nonfinite":                                        # ties among the finite ones too
        c = (rng.integers(0, 4, n) * 0.5).astype(f32)
        c[rng.random(n) < 0.3] = np.inf
        c[rng.random(n) < 0.2] = np.nan
        c[rng.random(n) < 0.1] = -np.inf
        c[::K] = 0.25                                                   # every group keeps a finite cost
        return c
    if case == "fewer_finite_than_elites":
        c = np.full(n, np.nan, f32)
        keep = max(1, elites - 1) if elites > 1 else 1
        for g in range(n // K):
            c[g * K + rng.permutation(K)[:keep]] = rng.random(keep).astype(f32)
        return c
    assert case == "none_finite"
    c = np.full(n, np.inf, f32)
    c[1::2] = np.nan
    return c


# ------------------------------------------------------------------ 1. sample is the stated function
@pytest.mark.parametrize("K", [5, 70])          # a partial wave; more than one wave
def test_sample_is_the_stated_function(models, K):
    rig = Rig(models["cfg3"], K, elites=3, alpha=0.7, env_offset=11)
    rng = np.random.default_rng(K)
    try:
        mean, sigma = rig.state()[:2]
        m0, s0 = ref.reset_state(P, H, rig.lo, rig.hi, 0.5)
        assert bits_equal(mean, m0) and bits_equal(sigma, s0)           # a new planner is a reset one
        seen = []
        for call in (0, 2 ** 24 + 5):                                   # the second: call 256 wraps inside the 32-bit counter word
            for it in (0, 1):
                mean, sigma = rig.state()[:2]
                rig.plan.begin_dev()
                for h in range(H):
                    got = rig.sample(call, it, h)
                    assert bits_equal(got, rig.ref_sample(mean, sigma, call, it, h)), (call, it, h)
                    assert bits_equal(got[:, 0], ref.clamp(mean[:, h], rig.lo, rig.hi))          # candidate 0: the current mean
                    seen.append(got)
                rig.put("extra", rng.random(rig.N))
                rig.plan.add_cost_dev(rig.p("extra"))
                rig.plan.update_dev()                                    # mean and sigma move: the next iteration samples around them
        assert not bits_equal(seen[0], seen[H]) and not bits_equal(seen[0], seen[2 * H])
        assert len({a.tobytes() for a in seen}) == len(seen)
    finally:
        rig.close()


# ------------------------------------------------------------------ 2. accumulate and costs
@pytest.mark.parametrize("body", ["block0", "hand_l_distal_link"])      # the task's body (at rest: one cost per group); a body the actions move
def test_costs_follow_the_steps_and_a_public_replay(models, body):
    m = models["cfg3"]
    K, gamma = 5, 0.5
    rig = Rig(m, K, gamma=gamma, goal_body=m.body_id(body))
    acting, replay = BatchSim(m, P), BatchSim(m, rig.N)
    try:
        q0 = np.tile(m.qpos0, (P, 1)).astype(f32)
        q0[:, 7] = [0.0, 0.04, -0.03]; q0[:, 8] = [0.0, -0.02, 0.05]
        goal = np.array([[0.01, 0.0, 0.422], [0.3, 0.1, 0.422], [-0.2, 0.2, 0.5]], f32)      # env 0: inside the geofence at once
        acting.reset(qpos0=q0, mocap=goal)
        acting.step(np.zeros((P, m.nu), f32), SUB)                      # a state with velocities, warm start and collision caches
        snap = acting.snapshot(rig.N)
        snap.save()
        slot, envs = np.arange(rig.N, dtype=np.int32) // K, np.arange(rig.N, dtype=np.int32)
        snap.load(slot, envs, into=rig.sim)
        snap.load(slot, envs, into=replay)
        rig.plan.begin_dev()
        c_dev, c_pub, ctrls = ref.Costs(rig.N), ref.Costs(rig.N), []
        for h in range(H):
            ctrl = rig.sample(0, 0, h)
            ctrls.append(ctrl)
            rig.sim.step_dev(rig.p("ctrl"), SUB, rig.goal_body, GEOFENCE, None, None, rig.p("done"), None)
            rig.plan.accumulate_dev(h)
            done = rig.host("done")[0]
            c_dev.step(ref.dist(rig.sim.body_xpos(rig.goal_body), rig.sim.body_xpos(MOCAP_BODY)), done, rig.sim.bad_state()[0], h, gamma)
            _, _, done_pub, _ = replay.step(ctrl.reshape(rig.N, m.nu), SUB, rig.goal_body, GEOFENCE)
            c_pub.step(ref.dist(replay.body_xpos(rig.goal_body), replay.body_xpos(MOCAP_BODY)), done_pub, replay.bad_state()[0], h, gamma)
        J, reach = rig.state()[2:4]
        print("J", J.reshape(P, K), "reach", reach.reshape(P, K))
        assert np.isfinite(J).all()                                     # no candidate went bad
        assert bits_equal(J, c_dev.J) and np.array_equal(reach, c_dev.reach)
        assert bits_equal(J, c_pub.J) and np.array_equal(reach, c_pub.reach)          # exact fork plus batch independence
        if body == "block0":
            assert np.all(reach[:K] == 0) and np.all(reach[K:] == -1)   # group 0 reached the goal in its first step, the others never
        else:
            assert np.all(reach == -1) and all(len(np.unique(J[p * K:(p + 1) * K])) == K for p in range(P))      # every candidate its own cost
        assert len(np.unique(np.stack(ctrls)[:, 1].reshape(H, K, -1), axis=1)[0]) == K          # the candidates of a group played different actions
        rig.plan.update_dev()
        assert np.all(rig.state()[6] == 0)
    finally:
        rig.close(); acting.close(); replay.close()


# ------------------------------------------------------------------ 3. update on planted costs
@pytest.mark.parametrize("K,elites", [(5, 1), (5, 3), (5, 5), (70, 1), (70, 3), (70, 70)])
def test_update_on_planted_costs(models, K, elites):
    rig = Rig(models["cfg3"], K, elites=elites, alpha=0.6, min_std=0.05)
    rng = np.random.default_rng(1000 * K + elites)
    try:
        for call, case in enumerate(("distinct", "equal", "some_nonfinite", "fewer_finite_than_elites", "none_finite", "distinct")):
            mean, sigma, _, _, _, _, failed = rig.state()
            act = rig.sample_horizon(call, 0)
            costs = planted_costs(case, rng, rig.N, K, elites)
            rig.put("extra", costs)
            rig.plan.add_cost_dev(rig.p("extra"))
            rig.plan.update_dev()
            got_mean, got_sigma, J, _, best, best_cost, got_failed = rig.state()
            # J = 0 + x = x; a NaN keeps being one
            assert np.array_equal(np.isnan(J), np.isnan(costs)) and bits_equal(np.nan_to_num(J, nan=0), np.nan_to_num(costs, nan=0))
            want_mean, want_sigma, want_best, want_cost, want_failed = rig.ref_update(mean, sigma, act, costs, failed)
            assert np.array_equal(best, want_best) and bits_equal(best_cost, want_cost), case
            assert np.array_equal(got_failed, want_failed), case
            assert bits_equal(got_mean, want_mean), case                # implies the elite sets: another set gives another mean
            assert ulps(got_sigma, want_sigma).max() <= 1, case
            assert np.all(got_sigma >= (f32(0.05) * rig.half.astype(np.float64)).astype(f32))
            if case == "none_finite":
                assert bits_equal(got_mean, mean) and bits_equal(got_sigma, sigma) and np.all(got_failed == failed + 1)
                assert np.all(best == 0) and np.all(np.isposinf(best_cost))
            else:
                assert np.all(got_failed == failed)
                if elites > 1:                                          # (a lone elite may be candidate 0, the mean itself)
                    assert not bits_equal(got_mean, mean)
            if case == "equal":
                assert np.all(best == 0)                                # ties are broken by the index
    finally:
        rig.close()


# ------------------------------------------------------------------ 7. argument checks
def test_refused_calls_change_nothing(models):
    m = models["cfg3"]
    K = 5
    rig = Rig(m, K)
    other = BatchSim(m, P * K)
    try:
        rig.sample_horizon(0, 0)
        rig.put("extra", np.arange(rig.N))
        rig.plan.add_cost_dev(rig.p("extra"))
        rig.plan.update_dev()
        before = rig.state()
        base = dict(seed=1, env_offset=0, groups=P, samples=K, horizon=H, elites=2, goal_body=rig.goal_body, geofence=GEOFENCE, gamma=1.0, alpha=1.0,
                    init_std=0.5, min_std=0.05)
        bad_specs = [dict(groups=P + 1), dict(groups=0), dict(samples=1, groups=P * K), dict(samples=K + 1), dict(horizon=0), dict(horizon=65), dict(elites=0),
                     dict(elites=K + 1), dict(goal_body=-1), dict(goal_body=m.nbody), dict(goal_body=MOCAP_BODY), dict(gamma=-0.1), dict(gamma=1.5),
                     dict(gamma=float("nan")), dict(alpha=0.0), dict(alpha=1.5), dict(alpha=float("nan")), dict(init_std=0.0), dict(init_std=float("inf")),
                     dict(init_std=float("nan")), dict(min_std=-1.0), dict(min_std=float("inf")), dict(min_std=float("nan"))]
        for change in bad_specs:
            with pytest.raises(AssertionError, match="hsr_batch_plan_create"):
                rig.sim.plan(PlanSpec(**{**base, **change}))
        big = BatchSim(m, 1025)                                         # samples above 1024
        with pytest.raises(AssertionError, match="samples outside"):
            big.plan(PlanSpec(**{**base, "groups": 1, "samples": 1025}))
        big.close()
        other.set_goals([(rig.goal_body, m.body_id("hand_l_distal_link"), 0.1)])
        with pytest.raises(AssertionError, match="extra goal terms"):
            other.plan(PlanSpec(**base))
        for call in (lambda: rig.plan.sample_dev(0, 256, 0, rig.p("ctrl")), lambda: rig.plan.sample_dev(0, -1, 0, rig.p("ctrl")),
                     lambda: rig.plan.sample_dev(0, 0, H, rig.p("ctrl")), lambda: rig.plan.sample_dev(0, 0, -1, rig.p("ctrl")),
                     lambda: rig.plan.sample_dev(0, 0, 0, None), lambda: rig.plan.accumulate_dev(H), lambda: rig.plan.accumulate_dev(-1),
                     lambda: rig.plan.add_cost_dev(None), lambda: rig.plan.action_dev(None)):
            with pytest.raises(AssertionError, match="hsr_plan_"):
                call()
        rig.sim.set_goals([(rig.goal_body, m.body_id("hand_l_distal_link"), 0.1)])       # terms set after the planner was made
        with pytest.raises(AssertionError, match="extra goal terms"):
            rig.plan.accumulate_dev(0)
        rig.sim.set_goals([])
        after = rig.state()
        for a, b in zip(before, after):
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
        ctrl_before = rig.host("ctrl")[0]
        rig.plan.accumulate_dev(0)                                      # and the planner still works
        assert np.array_equal(rig.host("ctrl")[0], ctrl_before)
        # the batch goes first: the handle refuses everything but its own destruction
        rig.sim.close()
        with pytest.raises(AssertionError, match="destroyed"):
            rig.plan.begin_dev()
    finally:
        rig.close(); other.close()


# ------------------------------------------------------------------ 8. shift and reset
def test_shift_and_reset_with_masks(models):
    rig = Rig(models["cfg3"], 5, elites=2, alpha=1.0, init_std=0.3)
    try:
        rig.sample_horizon(0, 0)
        rig.put("extra", np.random.default_rng(8).random(rig.N))
        rig.plan.add_cost_dev(rig.p("extra"))
        rig.plan.update_dev()
        mean, sigma = rig.state()[:2]
        assert len(np.unique(mean[:, :, 0])) == P * H                   # every step of every group has its own mean now
        for mask in ([1, 0, 1], [0, 0, 0], None):
            if mask is not None:
                rig.put("mask", mask)
            rig.plan.shift_dev(None if mask is None else rig.p("mask"))
            mean, sigma = ref.shift(mean, sigma, mask, rig.lo, rig.hi, 0.3)
            got = rig.state()[:2]
            assert bits_equal(got[0], mean) and bits_equal(got[1], sigma), mask
        for mask in ([0, 1, 0], None):
            if mask is not None:
                rig.put("mask", mask)
            rig.plan.reset_dev(None if mask is None else rig.p("mask"))
            mean, sigma = ref.reset(mean, sigma, mask, rig.lo, rig.hi, 0.3)
            got = rig.state()[:2]
            assert bits_equal(got[0], mean) and bits_equal(got[1], sigma), mask
        rig.plan.action_dev(rig.p("action"))
        assert bits_equal(rig.host("action")[0], mean[:, 0])
        assert bits_equal(mean[0, 0], ref.clamp(np.zeros(rig.nu, f32), rig.lo, rig.hi)) and np.any(mean[0, 0] != 0)       # zero is clamped into the ctrl range
    finally:
        rig.close()


# ------------------------------------------------------------------ 4. - 6. the planner of an env
def make_env(m, n=P, **kw):
    kw.setdefault("goals", [GoalSpec("block0", GOAL, GEOFENCE)])
    env = VecHSREnv(model=m, n_envs=n, starts={"block0joint": BLOCK_START}, steps_per_action=SUB, **kw)
    env.seed(5)
    env.reset()
    return env


def test_plans_are_reproducible(models):
    m = models["cfg3"]
    env = make_env(m)
    opts = dict(samples=6, horizon=2, iterations=2, elites=2, seed=11)
    a, b, c = env.make_planner(**opts), env.make_planner(**opts), env.make_planner(**opts, env_offset=1)
    singles = [make_env(m, n=1, env_offset=p, n_global=P) for p in range(P)]
    solo = [e.make_planner(**opts) for e in singles]
    try:
        assert bits_equal(env.sim.get_state()[1], np.concatenate([e.sim.get_state()[1] for e in singles]))       # the same acting states
        for call in range(3):
            fresh = None if call != 1 else np.array([0, 1, 0])
            ua, ub, uc = (x.plan(fresh).cpu().numpy() for x in (a, b, c))
            assert ua.shape == (P, m.nu) and np.all(ua >= m.act_ctrlrange[:, 0]) and np.all(ua <= m.act_ctrlrange[:, 1])
            assert bits_equal(ua, ub), call                             # one seed, one result
            assert not bits_equal(ua, uc)                               # another env_offset, other draws
            assert bits_equal(a.costs(), b.costs()) and np.array_equal(a.best()[0], b.best()[0])
            for p in range(P):                                          # group p does not depend on P
                up = solo[p].plan(None if fresh is None else fresh[p:p + 1]).cpu().numpy()
                assert bits_equal(up, ua[p:p + 1]), (call, p)
                singles[p].step(ua[p])
            env.step(ua)
        assert a.call == 3 and np.all(a.failed == 0) and a.costs().shape == (P, 6) and a.reach_step().shape == (P, 6)
    finally:
        for x in (a, b, c, *solo):
            x.close()
        for e in (env, *singles):
            e.close()


def test_make_planner_needs_a_body_and_a_point(models):
    m = models["cfg3"]
    env = VecHSREnv(model=m, n_envs=P, steps_per_action=SUB)
    with pytest.raises(ValueError, match="a body and a point"):
        env.make_planner(samples=4, horizon=2)
    env.close()
    both = [GoalSpec("block0", GOAL, GEOFENCE), GoalSpec("block0", "hand_l_distal_link", 0.5)]
    env = make_env(m, goals=both)
    with pytest.raises(AssertionError, match="extra goal terms"):       # carried over to the planning batch, where the library refuses them
        env.make_planner(samples=4, horizon=2)
    env.close()
    env = make_env(m)
    for bad in (dict(samples=1), dict(samples=4, horizon=0), dict(samples=4, horizon=2, elites=5), dict(samples=4, horizon=2, alpha=0.0)):
        with pytest.raises(AssertionError, match="hsr_batch_plan_create"):      # what the library refuses, the planner refuses
            env.make_planner(**bad)
    env.close()


@pytest.mark.parametrize("auto_reset", [False, True])
def test_the_acting_env_never_notices_a_planner(models, auto_reset):
    m = models["cfg3"]
    kw = dict(auto_reset=True, max_episode_steps=2) if auto_reset else {}
    plain, planned = make_env(m, **kw), make_env(m, **kw)
    if auto_reset:
        plain.make_replay(8, seed=3); planned.make_replay(8, seed=3)
    planner = planned.make_planner(samples=5, horizon=2, iterations=2)
    rng = np.random.default_rng(9)
    lo, hi = m.act_ctrlrange[:, 0], m.act_ctrlrange[:, 1]
    try:
        for _ in range(3):
            action = rng.uniform(lo, hi, (P, m.nu)).astype(f32)
            planner.plan()                                              # its action is ignored
            want, got = plain.step(action), planned.step(action)
            assert bits_equal(got[0], want[0]) and bits_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
            assert np.array_equal(got[3]["substeps"], want[3]["substeps"])
            if auto_reset:
                assert bits_equal(got[3]["terminal_observation"], want[3]["terminal_observation"])
        t0, t1 = plain.sim.get_state(), planned.sim.get_state()
        assert all(bits_equal(x, y) for x, y in zip(t0, t1)) and bits_equal(plain.sim.get_warmstart(), planned.sim.get_warmstart())
    finally:
        planner.close(); plain.close(); planned.close()


def test_the_planner_moves_the_hand_towards_the_goal(models):
    """The left finger's distal link, a goal point 3 cm to its side: five env-steps on plan() end closer to the point than five env-steps of
    zero action do, in every env.  No margin: the inequality alone."""
    m = models["cfg3"]
    hand = m.body_id("hand_l_distal_link")
    probe = BatchSim(m, 1)
    probe.forward()
    rest = probe.body_xpos(hand)[0]
    probe.close()
    goal = (rest + np.array([0.005, 0.03, -0.0035])).astype(f32)
    envs = [VecHSREnv(model=m, n_envs=P, goals=[GoalSpec("hand_l_distal_link", goal, 0.002)], steps_per_action=SUB) for _ in range(2)]
    for e in envs:
        e.seed(1); e.reset()
    idle, acting = envs
    planner = acting.make_planner(samples=64, horizon=3, iterations=3)
    try:
        for _ in range(5):
            acting.step(planner.plan().cpu().numpy())
            idle.step(np.zeros((P, m.nu), f32))
        d_plan = np.linalg.norm(acting.sim.body_xpos(hand) - goal, axis=1)
        d_idle = np.linalg.norm(idle.sim.body_xpos(hand) - goal, axis=1)
        print("distance to the goal: planned", d_plan, "zero action", d_idle, "failed", planner.failed)
        assert np.all(planner.failed == 0) and np.all(d_idle < 0.05)    # the goal is centimetres away, not somewhere else
        assert np.all(d_plan < d_idle)
    finally:
        planner.close(); idle.close(); acting.close()
