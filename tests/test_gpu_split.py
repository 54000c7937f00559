"""Hand-over of hard envs inside a launch of the persistent kernel (persist.h, split_logic.h): a wave that finds two or more hard envs
among its own at a check point keeps the hardest and gives the others to workgroups that have finished (or, here, to extra workgroups
without a task).  That only decides WHO runs an env from WHICH substep on: every output and the whole state must be bit-identical to the
launch that does not split.  The tests force the split (threshold 0: every live env counts as hard, so every wave gives away all but one
env at its first check point) on 64 contact-rich envs - 16 waves - with 16 extra helpers, check points every 8 substeps of a 60-substep
env-step, and no hand-over with fewer than 8 substeps ahead."""
import numpy as np
import pytest

from hsr_env_amd import sim as hs
from test_gpu_parity import random_states

pytestmark = pytest.mark.gpu

N, SUBSTEPS, PERIOD, MIN_LEFT, HELPERS = 64, 60, 8, 8, 16


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """The last test hands torch tensors to step_dev: torch finds the GPU only if it looks for it before the library's first batch does
    (bench.py's order), so it looks before the module's first test."""
    import torch
    torch.cuda.is_available()


def run(m, q, v, ctrl, goal, body, fence, split, helpers=HELPERS, env_steps=2):
    """env_steps env-steps from (q, v); every output and state array of each, and the hand-overs of each launch"""
    n = len(q)
    sim = hs.BatchSim(m, n)
    assert sim.is_persistent()
    if split:
        assert sim.set_split(True, PERIOD, 0.0, MIN_LEFT, helpers)
    else:
        assert sim.set_split(False)
    sim.set_mocap(goal)
    sim.set_state(np.zeros(n), q, v)
    out, handed = [], []
    for _ in range(env_steps):
        obs, rew, done, ns = sim.step(ctrl, SUBSTEPS, body, fence)
        handed.append(sim.solo_handovers())
        t, qq, vv = sim.get_state()
        out += [obs, rew, done, ns, t, qq, vv, sim.get_warmstart(), sim.newton_trips()]
    assert not sim.bad_state()[1]
    sim.sync()                                      # a drained launch would be reported here
    sim.close()
    return out, handed


def same(a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), f"the split changed array {k % 9} of env-step {k // 9}: envs {np.unique(np.nonzero(x != y)[0])[:8]}"


@pytest.fixture(scope="module")
def case(models):
    m = models["cfg3"]
    rng = np.random.default_rng(77)
    q, v, ctrl = random_states(m, N + 3, rng)
    far = np.tile([5.0, 5.0, 5.0], (N + 3, 1)).astype(np.float32)      # a goal nobody reaches: every env runs the whole env-step
    return m, q, v, ctrl, far, m.body_id(m.block_body())


@pytest.fixture(scope="module")
def plain(case):
    m, q, v, ctrl, far, bid = case
    return run(m, q[:N], v[:N], ctrl[:N], far[:N], bid, 0.03, False)[0]


def test_forced_split_never_changes_a_result(case, plain):
    """Every wave wants to give away all but one env at its first check point (substep 8) and does as far as helpers are free: 16 hand-overs
    or more per launch (one per extra helper; more as helpers come free again), every output and state array bit-identical to the plain launch, and a second env-step from the handed-over state too (margins, stamps and warm starts
    travel through global memory)."""
    m, q, v, ctrl, far, bid = case
    out, handed = run(m, q[:N], v[:N], ctrl[:N], far[:N], bid, 0.03, True)
    print("hand-overs per launch:", handed)
    assert min(handed) >= 16
    same(plain, out)
    assert (plain[3] == SUBSTEPS).all()


def test_split_off_hands_nothing_over(case):
    """The switch, on a batch that has already handed envs over: with the split off the next launch counts none."""
    m, q, v, ctrl, far, bid = case
    sim = hs.BatchSim(m, N)
    assert sim.set_split(True, PERIOD, 0.0, MIN_LEFT, HELPERS)
    sim.set_state(np.zeros(N), q[:N], v[:N])
    sim.step(ctrl[:N], SUBSTEPS)
    assert sim.solo_handovers() >= 16
    assert sim.set_split(False)
    sim.step(ctrl[:N], SUBSTEPS)
    assert sim.solo_handovers() == 0
    sim.close()


def test_early_exits_of_donated_envs(case):
    """The goal of every env is where its hand is after 30 substeps, so the envs leave the env-step one after the other on the way there -
    more of them after the first check point than the 16 envs the waves keep, so some leave while a helper runs them.  nsteps and done
    (and everything else) must match the plain launch."""
    m, q, v, ctrl, far, bid = case
    hand = m.body_id("hand_l_distal_link")
    sim = hs.BatchSim(m, N)
    sim.set_state(np.zeros(N), q[:N], v[:N])
    sim.step(ctrl[:N], 30)
    goal = sim.body_xpos(hand).astype(np.float32)
    sim.close()
    ref, _ = run(m, q[:N], v[:N], ctrl[:N], goal, hand, 0.01, False, env_steps=1)
    done, ns = ref[2], ref[3]
    late = int((done & (ns > PERIOD)).sum())
    print(f"early exits: {int(done.sum())} of {N}, {late} after the first check point; nsteps {np.sort(ns)}")
    assert late > 16 and (ns[done] < SUBSTEPS).any()
    out, handed = run(m, q[:N], v[:N], ctrl[:N], goal, hand, 0.01, True, env_steps=1)
    assert handed[0] >= 16
    same(ref, out)


def test_no_helper_free(case):
    """64 copies of one env: all waves end together, nobody is free while anybody could donate (no extra helpers), and a donor never waits -
    the launch ends as the plain one does, with the same results and a clean sync."""
    m, q, v, ctrl, far, bid = case
    q1, v1, c1 = np.tile(q[:1], (N, 1)), np.tile(v[:1], (N, 1)), np.tile(ctrl[:1], (N, 1))
    ref, _ = run(m, q1, v1, c1, far[:N], bid, 0.03, False)
    out, handed = run(m, q1, v1, c1, far[:N], bid, 0.03, True, helpers=0)
    print("hand-overs per launch without extra helpers:", handed)
    same(ref, out)


def test_ragged_batch(case):
    """64 + 3 envs: the last wave holds three envs and an empty lane group."""
    m, q, v, ctrl, far, bid = case
    ref, _ = run(m, q, v, ctrl, far, bid, 0.03, False, env_steps=1)
    out, handed = run(m, q, v, ctrl, far, bid, 0.03, True, env_steps=1)
    assert handed[0] >= 16
    same(ref, out)


def test_cupboard(models):
    m = models["cupboard"]
    rng = np.random.default_rng(78)
    q, v, ctrl = random_states(m, N, rng)
    far = np.tile([5.0, 5.0, 5.0], (N, 1)).astype(np.float32)
    bid = m.body_id(m.block_body())
    ref, _ = run(m, q, v, ctrl, far, bid, 0.03, False, env_steps=1)
    out, handed = run(m, q, v, ctrl, far, bid, 0.03, True, env_steps=1)
    assert handed[0] >= 16
    same(ref, out)


def test_drain_flag_is_sticky_over_split_launches(case, plain):
    """A drained launch must be reported by the next synchronising call however many split launches were enqueued behind it, and those
    launches must end: with the flag up donors keep their envs and helpers leave.  Hook 32 of hsr_batch_set_debug raises the flag after a
    launch exactly as a spin's watchdog does (test_work_queue_watchdog_flag_is_sticky); nothing here makes a launch hang."""
    import torch
    from hsr_env_amd.sim import DependencyNotInstalled
    m, q, v, ctrl, far, bid = case
    dev = torch.device("cuda", 0)
    sim = hs.BatchSim(m, N)
    assert sim.set_split(True, PERIOD, 0.0, MIN_LEFT, HELPERS)
    sim.set_mocap(far[:N])
    sim.set_state(np.zeros(N), q[:N], v[:N])
    d_ctrl = torch.from_numpy(ctrl[:N].astype(np.float32)).to(dev)
    d_obs = torch.empty((N, m.nq + m.nv), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    sim.set_debug(32)
    sim.step_dev(d_ctrl.data_ptr(), SUBSTEPS, bid, 0.03, d_obs.data_ptr())         # "drained"
    sim.set_debug(0)
    sim.step_dev(d_ctrl.data_ptr(), SUBSTEPS, bid, 0.03, d_obs.data_ptr())         # a split launch behind it, flag up
    with pytest.raises(DependencyNotInstalled, match="work-queue"):
        sim.sync()
    sim.sync()                                      # reported once, then clear
    assert sim.solo_handovers() == 0                # the launch behind the flag kept its envs ...
    torch.cuda.synchronize()
    assert np.array_equal(d_obs.cpu().numpy(), plain[9])        # ... and computed the second env-step of the plain run
    sim.close()
