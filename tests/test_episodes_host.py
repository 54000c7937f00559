"""The episode layer without a GPU: the checker's Philox against the published known answers, the tables EpisodeSpec.from_env builds
against the slots VecHSREnv.new_state writes, and the refusal of a simulator handle that cannot run episodes."""
import numpy as np
import pytest

import episode_ref as ref
from hsr_env_amd.env import GoalSpec, VecHSREnv
from hsr_env_amd.episodes import EpisodeSpec
from hsr_env_amd.spaces import Box
from oracle_batch import OracleBatchSim


@pytest.mark.parametrize("ctr,key,want", [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xffffffff] * 4, [0xffffffff] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_restatement_reproduces_the_random123_known_answers(ctr, key, want):
    got = ref.philox4x32_10(np.array(ctr, np.uint32), key)
    assert " ".join(f"{int(x):08x}" for x in got) == want


def test_uniform_is_exact_at_the_ends_and_inside_the_range():
    w = np.array([0, 0xffffffff, 0x80000000, 0x000000ff], np.uint32)
    assert ref.uniform(w, 0.25, 0.25).tolist() == [0.25] * 4                     # lo == hi yields lo
    v = ref.uniform(w, -0.1, 0.2)
    assert v.dtype == np.float32 and np.all(v >= np.float32(-0.1)) and np.all(v <= np.float32(0.2))
    assert v[0] == np.float32(-0.1) and v[3] == np.float32(-0.1)               # the low 8 bits of a word do not count


@pytest.mark.parametrize("cfg", ["cfg2", "cfg4"])
def test_spec_tables_follow_new_state(models, cfg):
    m = models[cfg]
    nb = (m.nq - m.nu) // 7
    starts = {"slide_x": Box([-0.3], [0.4]), "block0joint": Box([-.1, -.2, .422, 1, 0, 0, 0], [.1, .2, .5, 1, 0, 0, 0])}
    goal = Box([-.1, -.2, .422], [.1, .2, .422])
    spec = EpisodeSpec.from_env(m, starts, [GoalSpec("block0", goal, .05)], None, seed=2 ** 40 + 7, env_offset=5, max_episode_steps=9)
    q0 = m.qpos0.astype(np.float32)
    sx = m.joint_qpos_addr("slide_x")
    b0, b1 = m.joint_qpos_addr("block0joint")
    sampled = np.zeros(m.nq, bool); sampled[sx] = True; sampled[b0:b1] = True
    assert np.array_equal(spec.qpos_lo[~sampled], q0[~sampled]) and np.array_equal(spec.qpos_hi[~sampled], q0[~sampled])
    assert spec.qpos_lo[sx] == np.float32(-0.3) and spec.qpos_hi[sx] == np.float32(0.4)
    assert np.array_equal(spec.qpos_lo[b0:b1], np.float32([-.1, -.2, .422, 1, 0, 0, 0])) and np.array_equal(spec.qpos_hi[b0:b1], np.float32([.1, .2, .5, 1, 0, 0, 0]))
    assert (spec.seed, spec.env_offset, spec.max_episode_steps) == (2 ** 40 + 7, 5, 9)
    assert spec.has_goal and np.array_equal(spec.goal_lo, goal.low) and np.array_equal(spec.goal_hi, goal.high)
    assert len(spec.block_qadr) == 0
    # block_space: the slots are the ones new_state writes - the entries that differ from qpos0 when only block_space is given
    bs = Box([-.1, -.2, .5, -3.14], [.1, .2, .6, 3.14])
    spec = EpisodeSpec.from_env(m, {}, None, bs, seed=1)
    env = VecHSREnv(model=m, n_envs=2, sim=OracleBatchSim(m, 2), block_space=bs)
    moved = np.flatnonzero(np.any(env.new_state() != m.qpos0, axis=0))
    slots = np.concatenate([np.arange(a, a + 7) for a in spec.block_qadr])
    assert len(spec.block_qadr) == nb and set(moved) <= set(slots) and {int(a) + 2 for a in spec.block_qadr} <= set(moved)
    assert list(spec.block_qadr) == m.free_joint_qadrs()
    assert not spec.has_goal and np.array_equal(spec.block_lo, bs.low) and np.array_equal(spec.block_hi, bs.high)
    assert np.array_equal(spec.qpos_lo, q0) and np.array_equal(spec.qpos_hi, q0)
    # a fixed goal point is a range of width zero
    spec = EpisodeSpec.from_env(m, {}, [GoalSpec("block0", np.array([.4, 0, .422]), .05)], None)
    assert spec.has_goal and np.array_equal(spec.goal_lo, np.float32([.4, 0, .422])) and np.array_equal(spec.goal_lo, spec.goal_hi)
    c, keep = spec.to_c()
    assert (c.nblock, c.has_goal, c.max_episode_steps) == (0, 1, 0) and [c.qpos_lo[i] for i in range(m.nq)] == q0.tolist()


def test_spec_refuses_what_the_device_cannot_sample(models):
    m = models["cfg2"]
    with pytest.raises(ValueError):
        EpisodeSpec.from_env(m, {"slide_x": Box([-np.inf], [1.0])})
    with pytest.raises(ValueError):
        EpisodeSpec.from_env(m, {}, [GoalSpec("block0", Box([-1, -1, -np.inf], [1, 1, np.inf]), .05)])
    with pytest.raises(ValueError):
        EpisodeSpec.from_env(m, {}, None, Box([-1, -1, 0, -np.inf], [1, 1, 1, np.inf]))
    with pytest.raises(ValueError):
        EpisodeSpec.from_env(m, {"no_such_joint": Box([0.], [1.])})
    with pytest.raises(ValueError):
        EpisodeSpec.from_env(m, {"block0joint": Box([0.], [1.])})                # a Box of one value for a slice of seven


def test_books_restatement_counts_returns_lengths_and_truncations(models):
    spec = EpisodeSpec.from_env(models["cfg2"], {}, None, None, seed=3, max_episode_steps=2)
    bk = ref.Books(spec, np.arange(3))
    bk.begin()
    assert bk.index.tolist() == [1, 1, 1]
    kind, r, l, _, _ = bk.end([0, 1, 0], [False, True, False])
    assert kind.tolist() == [0, 1, 0] and r.tolist() == [0, 1, 0] and l.tolist() == [0, 1, 0] and bk.index.tolist() == [1, 2, 1]
    kind, r, l, _, _ = bk.end([0, 0, 1], [False, False, True])
    assert kind.tolist() == [2, 0, 1] and r.tolist() == [0, 0, 1] and l.tolist() == [2, 0, 2] and bk.length.tolist() == [0, 1, 0]


def test_auto_reset_needs_a_device_handle(models):
    m = models["cfg2"]
    with pytest.raises(NotImplementedError):
        VecHSREnv(model=m, n_envs=2, sim=OracleBatchSim(m, 2), auto_reset=True, max_episode_steps=3)
    with pytest.raises(ValueError):
        VecHSREnv(model=m, n_envs=2, sim=OracleBatchSim(m, 2), max_episode_steps=3)      # a time limit without the episode layer
