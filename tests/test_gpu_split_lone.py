"""The lone rule of the hand-over inside a launch (persist.h, split_logic.h: split_decide_lone): a wave whose one hard env still has easier
live neighbours gives that env to a workgroup that has finished (here: to extra workgroups without a task) and goes on with the
neighbours.  As with the two-hard rule that only decides WHO runs an env from WHICH substep on: every output and the whole state must be
bit-identical to the launch that does not split.  The batch is 16 waves of one contact-rich env in lane group 0 - random states as in
test_gpu_split.py, advanced 300 substeps under their ctrl so that the arm has reached what it presses on; of a pool of 256 the ones a plain
launch found hardest over the test's 60 substeps - and three copies of one easy env - block at rest on the table, base slid away from it,
arm up, ctrl that holds that pose - in groups 1-3; the two-hard threshold is 1000 (it never fires), the lone threshold lies between the two classes, check points every 8
substeps of a 60-substep env-step, no hand-over with fewer than 8 substeps ahead, 16 extra helpers."""
import numpy as np
import pytest

from hsr_env_amd import sim as hs
from test_gpu_parity import random_states

pytestmark = pytest.mark.gpu

N, WAVES, SUBSTEPS, PERIOD, MIN_LEFT, HELPERS = 64, 16, 60, 8, 8, 16
SEED, POOL, ADVANCE = 77, 256, 300      # the pool of random states (test_gpu_split.py's seed) and the substeps that bring them into contact
TWO_HARD = 1000.0           # Newton iterations per substep nobody reaches: only the lone rule donates
LONE = 1.5                  # between the classes (iterations per substep of the plain launch, first env-step: easy copies 1.0, rich envs 1.7 and more)


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch finds the GPU only if it looks for it before the library's first batch does (as in test_gpu_split.py)."""
    import torch
    torch.cuda.is_available()


def easy_env(m):
    """One easy env: the block at rest in a corner of the table, the base slid to the opposite end of its travel, the arm lifted and
    flexed as little as the actuators allow, and the ctrl whose set points are exactly that pose (force = kp * (ctrl - gear * q))."""
    q = np.array(m.qpos0, dtype=np.float64)
    pose = {"slide_x": -0.12, "slide_y": -0.22, "arm_lift_joint": 0.31, "arm_flex_joint": -0.5}
    qa, da = m.scalar_joints()
    names = m.names["joint"]
    for name, val in pose.items():
        q[qa[names.index(name)]] = val
    a = m.free_joint_qadrs()[0]
    q[a:a + 3] = [0.1, 0.2, 0.422]
    ctrl = np.zeros(m.nu)
    for k in range(m.nu):
        j = list(da).index(m.act_dof[k])
        ctrl[k] = np.clip(m.act_gear[k] * q[qa[j]], m.act_ctrlrange[k, 0], m.act_ctrlrange[k, 1])
    return q, np.zeros(m.nv), ctrl


def rich_envs(m, count, seed=SEED):
    """the `count` hardest of POOL random states advanced by ADVANCE substeps: hardest by the Newton iterations of a plain launch (no
    split) over the SUBSTEPS substeps the tests run from that state"""
    rng = np.random.default_rng(seed)
    q, v, ctrl = random_states(m, POOL, rng)
    far = np.tile([5.0, 5.0, 5.0], (POOL, 1)).astype(np.float32)
    bid = m.body_id(m.block_body())
    trips = None
    for substeps in (ADVANCE, SUBSTEPS):
        sim = hs.BatchSim(m, POOL)
        assert sim.set_split(False)
        sim.set_mocap(far)
        sim.set_state(np.zeros(POOL), q, v)
        sim.step(ctrl, substeps, bid, 0.03)
        assert not sim.bad_state()[1]
        if substeps == ADVANCE:
            _, q, v = sim.get_state()
        else:
            trips = sim.newton_trips()
        sim.close()
    pick = np.argsort(-trips, kind="stable")[:count]
    return q[pick], v[pick], ctrl[pick]


def batch(m, seed=SEED, extra=0):
    """envs 0-15 contact-rich, 16-63 copies of the easy env: the first launch packs env w into lane group 0 of wave w and fills the other
    groups from the far end (hsr_batch_packing's contract with every iteration count still zero); `extra` more rich envs at the end"""
    qr, vr, cr = rich_envs(m, WAVES + extra, seed)
    qe, ve, ce = easy_env(m)
    q = np.concatenate([qr[:WAVES], np.tile(qe, (N - WAVES, 1)), qr[WAVES:]])
    v = np.concatenate([vr[:WAVES], np.tile(ve, (N - WAVES, 1)), vr[WAVES:]])
    ctrl = np.concatenate([cr[:WAVES], np.tile(ce, (N - WAVES, 1)), cr[WAVES:]])
    return q, v, ctrl


def run(m, q, v, ctrl, goal, body, fence, lone, helpers=HELPERS, env_steps=2, split=True):
    """env_steps env-steps from (q, v); every output and state array of each, the hand-overs of each launch, the packing of the first"""
    n = len(q)
    sim = hs.BatchSim(m, n)
    assert sim.is_persistent()
    assert sim.set_split(split, PERIOD, TWO_HARD, MIN_LEFT, helpers)
    assert sim.set_split_lone(lone, LONE)
    sim.set_mocap(goal)
    sim.set_state(np.zeros(n), q, v)
    out, handed, packing = [], [], None
    for k in range(env_steps):
        obs, rew, done, ns = sim.step(ctrl, SUBSTEPS, body, fence)
        handed.append(sim.solo_handovers())
        if k == 0:
            packing = sim.packing(4)
        t, qq, vv = sim.get_state()
        out += [obs, rew, done, ns, t, qq, vv, sim.get_warmstart(), sim.newton_trips()]
    assert not sim.bad_state()[1]
    sim.sync()                                      # a drained launch would be reported here
    sim.close()
    return out, handed, packing


def same(a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), f"the split changed array {k % 9} of env-step {k // 9}: envs {np.unique(np.nonzero(x != y)[0])[:8]}"


@pytest.fixture(scope="module")
def case(models):
    m = models["cfg3"]
    q, v, ctrl = batch(m, extra=3)
    far = np.tile([5.0, 5.0, 5.0], (N + 3, 1)).astype(np.float32)      # a goal nobody reaches: every env runs the whole env-step
    return m, q, v, ctrl, far, m.body_id(m.block_body())


@pytest.fixture(scope="module")
def plain(case):
    """the launch that does not split at all: the reference of every case, and the premise - read from it, not from the code under test"""
    m, q, v, ctrl, far, bid = case
    out, handed, packing = run(m, q[:N], v[:N], ctrl[:N], far[:N], bid, 0.03, False, split=False)
    assert handed == [0, 0]
    per_sub = out[8] / SUBSTEPS                     # Newton iterations per substep over the first env-step
    print("plain launch, iterations per substep: rich", np.round(per_sub[:WAVES], 2), "easy", np.round(per_sub[WAVES:].max(), 2))
    assert (per_sub[:WAVES] >= LONE).sum() >= 12, "premise: at least 12 of the 16 rich envs at or above the lone threshold"
    assert (per_sub[WAVES:] <= LONE - 0.3).all(), "premise: every easy copy below the lone threshold by 0.3 iterations per substep or more"
    assert (packing[:, 0] == np.arange(WAVES)).all() and (packing[:, 1:] >= WAVES).all(), "premise: one rich env per wave, in lane group 0"
    assert (out[3] == SUBSTEPS).all()
    return out


def test_lone_rule_never_changes_a_result(case, plain):
    """Every wave whose rich env ran at the threshold over a window gives it to a helper: 8 hand-overs or more in the first launch (the
    rule is not inert), every output and state array of two env-steps bit-identical to the plain launch - the second env-step starts
    from handed-over state."""
    m, q, v, ctrl, far, bid = case
    out, handed, packing = run(m, q[:N], v[:N], ctrl[:N], far[:N], bid, 0.03, True)
    print("hand-overs per launch:", handed)
    assert handed[0] >= 8
    assert (packing[:, 0] == -1).sum() == handed[0] and (packing[:, 1:] >= WAVES).all()      # the rich envs left, their neighbours stayed
    same(plain, out)


def test_lone_rule_off_hands_nothing_over(case, plain):
    """The split on, the lone rule off, the two-hard threshold out of reach: no hand-over, the plain launch's results."""
    m, q, v, ctrl, far, bid = case
    out, handed, _ = run(m, q[:N], v[:N], ctrl[:N], far[:N], bid, 0.03, False)
    assert handed == [0, 0]
    same(plain, out)


def test_early_exits_of_donated_envs(case):
    """The goal of every rich env is where its hand is after 30 substeps (test_gpu_split.py's placement; the fence is 3 mm, not 10: these
    arms are pressing on something and move slowly), so rich envs leave the env-step on the way there, some of them on the helper that took
    them over; the easy copies keep the goal nobody reaches, so that the waves have live neighbours to leave.  nsteps, done and
    everything else must match the plain launch."""
    m, q, v, ctrl, far, bid = case
    hand = m.body_id("hand_l_distal_link")
    sim = hs.BatchSim(m, N)
    sim.set_state(np.zeros(N), q[:N], v[:N])
    sim.step(ctrl[:N], 30)
    goal = far[:N].copy()
    goal[:WAVES] = sim.body_xpos(hand).astype(np.float32)[:WAVES]
    sim.close()
    ref, _, _ = run(m, q[:N], v[:N], ctrl[:N], goal, hand, 0.003, False, env_steps=1, split=False)
    done, ns = ref[2], ref[3]
    late = int((done[:WAVES] & (ns[:WAVES] > PERIOD)).sum())
    print(f"early exits: {int(done.sum())} of {N}, {late} rich envs after the first check point; nsteps of the rich envs {np.sort(ns[:WAVES])}")
    assert late >= 8 and (ns[:WAVES][done[:WAVES]] < SUBSTEPS).any() and not done[WAVES:].any()
    out, handed, packing = run(m, q[:N], v[:N], ctrl[:N], goal, hand, 0.003, True, env_steps=1)
    gone = packing[:, 0] == -1
    print("hand-overs:", handed, "of them done early:", int((done[:WAVES] & gone).sum()))
    assert handed[0] >= 1 and (done[:WAVES] & gone).any()      # an env finished early on its helper
    same(ref, out)


def test_no_helper_free(case, plain):
    """No extra helpers: every wave runs all 60 substeps, so the only helpers are the waves with the easiest rich envs, late in the
    launch; most donors find no credit and never wait - the launch ends as the plain one does, with the same results and a clean sync
    (run() ends with it)."""
    m, q, v, ctrl, far, bid = case
    out, handed, _ = run(m, q[:N], v[:N], ctrl[:N], far[:N], bid, 0.03, True, helpers=0)
    print("hand-overs per launch without extra helpers:", handed)
    same(plain, out)


def test_ragged_batch(case):
    """64 + 3 envs: the last wave holds three envs and an empty lane group."""
    m, q, v, ctrl, far, bid = case
    ref, _, _ = run(m, q, v, ctrl, far, bid, 0.03, False, env_steps=1, split=False)
    out, handed, _ = run(m, q, v, ctrl, far, bid, 0.03, True, env_steps=1)
    print("hand-overs, ragged:", handed)
    assert handed[0] >= 8
    same(ref, out)
