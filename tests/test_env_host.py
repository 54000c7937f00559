"""Host-side mirror of HSREnv / MujocoEnv (hsr/env.py, hsr/mujoco_env.py) exercised on CPU through the
oracle-backed stand-in of BatchSim (tests/oracle_batch.py)."""
import numpy as np
import pytest

from hsr_env_amd import GoalSpec, VecHSREnv, Box
from hsr_env_amd import util
from hsr_env_amd.env import block_space_to_qpos, distance_between
from oracle_batch import mat2euler
from oracle_batch import OracleBatchSim


def make_env(models, cfg="cfg2", n=1, **kw):
    m = models[cfg]
    return VecHSREnv(model=m, n_envs=n, sim=OracleBatchSim(m, n), **kw)


def test_single_env_contract_matches_reference_shapes(models):
    """N = 1: obs[nq+nv], float reward, bool done, info keys of hsr/env.py:133-135; control.py loop runs."""
    env = make_env(models, "cfg1", 1, goals=None, starts={}, steps_per_action=5)
    assert env.action_space.shape == (2,) and np.allclose(env.action_space.low, [-1, -1])    # world.xml:106,109
    assert env.observation_space.shape == (4,) and env.obs_dim == 4
    done = False
    for _ in range(3):                                   # hsr/control.py:73-76
        if done:
            env.reset()
        s, r, t, i = env.step(np.zeros(2))
        done = t
        assert s.shape == (4,) and isinstance(r, float) and isinstance(t, bool)
        assert set(i["log count"]) == {"success"}
    assert not done                                        # goals is None -> done stays False (hsr/env.py:125)
    assert abs(env.dt - 0.002 * 20) < 1e-12               # frame_skip = record_freq default 20 (hsr/env.py:54,68)


def test_goal_reset_and_early_exit(models):
    m = models["cfg2"]
    goal_space = Box(low=[-.1, -.2, .422], high=[.1, .2, .422])
    block_space = Box(low=[-.1, -.2, .422, -3.14], high=[.1, .2, .422, 3.14])
    env = make_env(models, "cfg2", 8, goals=[GoalSpec("block0", goal_space, 0.5)], block_space=block_space, steps_per_action=30)
    env.seed(3)
    obs = env.reset()
    assert obs.shape == (8, 17)
    # block pose was sampled from block_space, goal from goal_space and written to mocap_pos (hsr/env.py:169)
    assert (np.abs(obs[:, 2]) <= .1).all() and np.allclose(obs[:, 4], .422) and np.allclose(np.linalg.norm(obs[:, 5:9], axis=1), 1)
    assert np.allclose(env.sim.body_xpos(m.body_id("goal")), env._goal_points)
    # geofence .5 covers the whole pan: success at the first substep, obs is the state at that substep
    obs, rew, done, info = env.step(np.zeros((8, 2)))
    assert done.all() and (rew == 1).all() and (info["substeps"] == 1).all()
    assert env.in_range("block0", env._goal_points, 0.5).all()
    env2 = make_env(models, "cfg2", 8, goals=[GoalSpec("block0", np.array([.4, 0, .422]), 0.05)], steps_per_action=30)
    env2.reset()
    obs, rew, done, info = env2.step(np.zeros((8, 2)))
    assert (not done.any()) and (info["substeps"] == 30).all()


def test_starts_sample_joint_slices(models):
    """hsr/__init__.py:14-18: starts={'blockjoint': Box(7)} resamples that joint's qpos slice at reset."""
    m = models["cfg2"]
    box = Box(low=[-.1, -.2, .43, 1, 0, 0, 0], high=[.1, .2, .43, 1, 0, 0, 0])
    env = make_env(models, "cfg2", 4, goals=[GoalSpec("block0", np.array([0, 0, .498]), .05)], starts={"block0joint": box})
    obs = env.reset()
    assert np.allclose(obs[:, 4], .43) and np.allclose(obs[:, 5:9], [1, 0, 0, 0]) and np.ptp(obs[:, 2]) > 0
    assert np.allclose(env.block_pos(), obs[:, 2:5], atol=1e-6)
    g = env.gripper_pos()
    assert g.shape == (4, 3)


def test_masked_reset_keeps_other_envs(models):
    env = make_env(models, "cfg2", 4, goals=None, steps_per_action=10)
    env.reset()
    env.step(np.ones((4, 2)))
    before = env._get_observation().copy()
    env.reset(mask=[True, False, True, False])
    after = env._get_observation()
    assert np.array_equal(after[[1, 3]], before[[1, 3]]) and np.allclose(after[[0, 2], :2], 0)


def test_sharded_sampling_reproduces_single_process(models):
    """Rank r of W draws the global batch and keeps [r*N/W, (r+1)*N/W): shards concatenate to the 1-GPU run."""
    m = models["cfg2"]
    gs = Box(low=[-.1, -.2, .422], high=[.1, .2, .422]); bs = Box(low=[-.1, -.2, .422, -3], high=[.1, .2, .422, 3])
    full = VecHSREnv(model=m, n_envs=6, sim=OracleBatchSim(m, 6), goals=[GoalSpec("block0", gs, .05)], block_space=bs)
    full.seed(7); o_full = full.reset()
    parts = []
    for r in range(2):
        e = VecHSREnv(model=m, n_envs=3, sim=OracleBatchSim(m, 3), goals=[GoalSpec("block0", gs, .05)], block_space=bs,
                      env_offset=3 * r, n_global=6)
        e.seed(7); parts.append((e.reset(), e._goal_points.copy()))
    assert np.array_equal(np.concatenate([p[0] for p in parts]), o_full)
    assert np.array_equal(np.concatenate([p[1] for p in parts]), full._goal_points)


def test_set_state_shape_assertion(models):
    env = make_env(models, "cfg1", 1)
    with pytest.raises(AssertionError):
        env.set_state(np.zeros(3), np.zeros(2))           # hsr/mujoco_env.py:88-89
    env.set_state(np.array([.05, -.02]), np.zeros(2))
    assert np.allclose(env._get_observation()[:2], [.05, -.02])


def test_bad_goal_type_raises(models):
    with pytest.raises(RuntimeError):
        make_env(models, "cfg2", 1, goals=[GoalSpec(3.0, np.zeros(3), .1)])      # hsr/env.py:145


def test_cli_grammar():
    """rl_utils/argparse.py:62-73 space grammar and the reference's flag names (hsr/util.py:16-40)."""
    import argparse
    b = util.parse_space(3)("(-.1,.1)(-.2,.2)(.422,.422)")
    assert np.allclose(b.low, [-.1, -.2, .422]) and np.allclose(b.high, [.1, .2, .422])
    with pytest.raises(argparse.ArgumentTypeError):
        util.parse_space(4)("(0,1)(0,1)")
    parser = argparse.ArgumentParser()
    util.add_env_args(parser.add_argument_group("env_args")); util.add_wrapper_args(parser.add_argument_group("wrapper_args"))
    args = util.hierarchical_parse_args(parser, ["--steps-per-action=300", "--geofence=.5", "--goal-space", "(0,0)(0,0)(0,0)",
                                                 "--use-dof", "slide_x", "--use-dof", "slide_y"])
    assert args["env_args"]["steps_per_action"] == 300 and args["wrapper_args"]["use_dof"] == ["slide_x", "slide_y"]
    assert args["wrapper_args"]["n_blocks"] == 0 and args["wrapper_args"]["geofence"] == .5
    m = util.model_for(["slide_y", "slide_x"], 1)
    assert (m.nq, m.nv, m.nu) == (9, 8, 2)


def test_math_helpers():
    assert np.allclose(block_space_to_qpos(np.array([.1, .2, .3, np.pi / 2])), [.1, .2, .3, np.cos(np.pi / 4), 0, 0, np.sin(np.pi / 4)])
    c, s = np.cos(.3), np.sin(.3)
    assert np.allclose(mat2euler(np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])), [0, 0, .3])
    assert distance_between(np.zeros(3), np.array([3., 4, 0])) == 5


def test_init_demo_shape_runs_on_the_cupboard_scene(models):
    """hsr/__init__.py:10-27 verbatim in shape: GoalSpec(a='block', b=point, distance=.05), starts={'blockjoint': Box(7)},
    random actions, reset when done - the body / joint names exist as such only in cupboard-world.xml:113-116."""
    m = models["cupboard"]
    starts = dict(blockjoint=Box(low=np.array([-.1, -.2, .418, 0, 0, -1, 0]), high=np.array([.1, +.2, .418, 1, 0, +1, 0])))
    env = make_env(models, "cupboard", 2, goals=[GoalSpec(a="block", b=np.array([0, 0, .498]), distance=.05)], starts=starts,
                   steps_per_action=10)
    env.seed(0)
    obs = env.reset()
    a0, a1 = m.joint_qpos_addr("blockjoint")
    assert (a0, a1) == (0, 7) and obs.shape == (2, 27)             # the block's free joint comes first in this scene
    assert (np.abs(obs[:, 0]) <= .1).all() and (np.abs(obs[:, 1]) <= .2).all() and np.allclose(obs[:, 2], .418)
    for _ in range(3):
        action = np.stack([env.action_space.sample() for _ in range(2)])
        s, r, t, i = env.step(action)
        assert s.shape == (2, 27) and np.isfinite(s).all() and not t.any()
    assert np.allclose(env.block_pos(), env.sim.body_xpos(m.body_id("block")))


def test_cli_set_xml_and_xml_file(models, monkeypatch, tmp_path):
    """hsr/util.py:36-37,43-44,129-135: `--xml-file`, `--set-xml path,value` (last path component = attribute, the rest an
    ElementTree path in whichever file it matches).  A known config resolves to its committed blob; a setter needs the
    model compiler and the MJCF / STL data files (the stored copies under tests/golden/hsr_data stand in for them)."""
    import argparse
    import functools
    from pathlib import Path
    from hsr_env_amd import compiler as hc
    parser = argparse.ArgumentParser()
    util.add_env_args(parser.add_argument_group("env_args")); util.add_wrapper_args(parser.add_argument_group("wrapper_args"))
    args = util.hierarchical_parse_args(parser, ["--steps-per-action=300", "--geofence=.05", "--goal-space", "(0,0)(0,0)(.498,.498)",
                                                 "--xml-file", "models/cupboard-world.xml", "--set-xml", "option/timestep,0.001",
                                                 "--set-xml", "body/joint[@name='slide_x']/damping,1000"]
                                        + sum([["--use-dof", d] for d in util.ALL_DOFS], []))
    w = args["wrapper_args"]
    assert w["set_xml"] == [util.XMLSetter("option/timestep", "0.001"), util.XMLSetter("body/joint[@name='slide_x']/damping", "1000")]
    m = util.model_for(w["use_dof"], w["n_blocks"], w["xml_file"])
    assert m.to_bytes() == models["cupboard"].to_bytes()
    # without the data files a setter is an IOError
    monkeypatch.setattr(util, "DEFAULT_REF_ROOT", tmp_path / "missing")
    with pytest.raises(IOError):
        util.model_for(w["use_dof"], w["n_blocks"], w["xml_file"], w["set_xml"])
    ref_data = Path(__file__).parent / "golden" / "hsr_data"
    monkeypatch.setattr(util, "DEFAULT_REF_ROOT", ref_data)
    monkeypatch.setattr(util, "compile_model", functools.partial(hc.compile_model, ref_root=ref_data))
    m2 = util.model_for(w["use_dof"], w["n_blocks"], w["xml_file"], w["set_xml"])
    assert m2.timestep == 0.001 and m2.meta["set_xml"][0] == ["option/timestep", "0.001"]
    i = m2.meta["dofs"].index("slide_x")
    qa, da = m2.scalar_joints()
    assert m2.dof_damping[da[i]] == 1000 and m2.dof_damping[da[i + 1]] == 2200          # hsr.mjcf:4,6
    assert np.array_equal(m2.arrays["pair_geom1"], models["cupboard"].arrays["pair_geom1"])


def test_openai_obs_type_shapes(models):
    """obs_type='openai' (hsr/env.py:72-110): 25-dim observation from reset() and step(); needs finger joints + a block."""
    env = make_env(models, "cfg3", 2, goals=[GoalSpec("block0", np.array([0, 0, .498]), .05)], obs_type="openai", steps_per_action=5)
    assert env.obs_dim == 25 and env.observation_space.shape == (25,)
    obs = env.reset()
    assert obs.shape == (2, 25) and np.isfinite(obs).all()
    assert np.allclose(obs[:, 6:9], obs[:, 3:6] - obs[:, 0:3], atol=1e-6)          # object_rel_pos = object_pos - grip_pos
    assert np.allclose(obs[:, 0:3], env.gripper_pos(), atol=1e-6) and np.allclose(obs[:, 3:6], env.block_pos(), atol=1e-6)
    with pytest.raises(ValueError):
        make_env(models, "cfg2", 1, obs_type="openai")                                # no finger joints among the DOFs


def test_control_loop_on_the_stand_in(models, capsys):
    """hsr/control.py:48-76 on the product's driver (hsr_env_amd/control.py): ControlHSREnv.control_agent steps with the zero action and returns
    `done`; the loop resets the finished envs by mask and goes on.  Geofence .5 around the goal covers the pan (README.md:5 uses the same
    value), so every env finishes on its first substep and is reset before the next env-step."""
    from hsr_env_amd import control
    m = models["cfg2"]
    goal_space = Box(low=[-.1, -.2, .422], high=[.1, .2, .422])
    block_space = Box(low=[-.1, -.2, .422, -3.14], high=[.1, .2, .422, 3.14])
    env = control.ControlHSREnv(model=m, n_envs=4, sim=OracleBatchSim(m, 4), goals=[GoalSpec("block0", goal_space, 0.5)], block_space=block_space, steps_per_action=300)
    env.seed(1)
    env.reset()
    t = env.control_agent()
    assert t.shape == (4,) and t.all()
    resets = []
    orig = env.reset
    env.reset = lambda mask=None: (resets.append(np.array(mask).copy()), orig(mask=mask))[1]
    k, dt = control.run(env, env_steps=3)
    assert k == 3 and len(resets) == 2 and all(r.all() for r in resets)        # no reset before the first env-step (done starts False), one before each of the others
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert line.startswith("3 env-steps x 4 envs in ") and line.endswith("env-steps/s")
    # a goal out of reach: nobody finishes, nothing is reset, 300 substeps each
    env2 = control.ControlHSREnv(model=m, n_envs=2, sim=OracleBatchSim(m, 2), goals=[GoalSpec("block0", np.array([.4, 0, .422]), 0.05)], steps_per_action=20)
    env2.reset()
    resets2 = []
    orig2 = env2.reset
    env2.reset = lambda mask=None: (resets2.append(mask), orig2(mask=mask))[1]
    control.run(env2, env_steps=2, random_actions=True)
    assert not resets2
    # N = 1 keeps the reference's scalar shapes through the same loop
    env1 = control.ControlHSREnv(model=models["cfg1"], n_envs=1, sim=OracleBatchSim(models["cfg1"], 1), goals=None, starts={}, steps_per_action=5)
    env1.reset()
    assert env1.control_agent() is False
    control.run(env1, env_steps=2)


def test_readme_command_line_selects_baseline_config_1(models):
    """README.md:5 / BASELINE config 1: the reference's literal flags parse into the slide_x / slide_y model without a block and no goal."""
    import argparse
    parser = argparse.ArgumentParser()
    wrapper_parser = parser.add_argument_group('wrapper_args')
    env_parser = parser.add_argument_group('env_args')
    util.add_env_args(env_parser)
    util.add_wrapper_args(wrapper_parser)
    argv = ["--block-space", "(0,0)(0,0)(0,0)(0,0)", "--steps-per-action=300", "--geofence=.5", "--goal-space", "(0,0)(0,0)(0,0)", "--use-dof", "slide_x", "--use-dof", "slide_y"]
    args = util.hierarchical_parse_args(parser, argv)
    got = {}
    util.env_wrapper(lambda env_args, **kw: got.update(env_args))(**args)
    assert got["steps_per_action"] == 300 and got["goals"] is None and got["block_space"] is None
    assert got["model"].nv == 2 and got["model"].nu == 2 and not got["model"].block_body()


# ------------------------------------------------------------------ the rules of auto_reset=True, on a scripted device loop
class EpisodeStandIn(OracleBatchSim):
    """The stand-in with an episode layer that does nothing: the scripted loop below says which envs were reset."""

    def set_episodes(self, spec):
        pass

    def reset_sampled(self, mask=None):
        pass

    def move_goal(self, point):
        self.reset(mocap=np.tile(np.float32(point), (self.n, 1)))


class ScriptedLoop:
    """In place of device_loop.DeviceLoop: step() hands out prepared records and, as DeviceLoop.step does between the step and the
    episode end, tells the recorder what the step latched."""
    replay = None

    def __init__(self, sim, records):
        self.sim, self.records = sim, list(records)

    def reset(self, mask):
        pass

    def commit_host_rows(self, obs, mask=None):
        pass

    def step(self, action, steps, goal_body, geofence, openai, recorder):
        r = self.records.pop(0)
        self.sim.last = (r.nsteps, steps)                  # what FakeCaptureSim.step leaves for its capture calls
        self.sim.steps = getattr(self.sim, "steps", 0) + 1
        if recorder is not None:
            recorder.after_step(r.done.astype(bool), r.nsteps)
        return r


def scripted_records(n, dim, steps=20):
    from hsr_env_amd.device_loop import StepRecord
    rng = np.random.default_rng(5)
    kinds = np.array([[0, 0, 0], [1, 0, 2], [2, 1, 0]], np.uint8)[:, :n]       # env 0 alone meets 0, 1 and 2
    return [StepRecord(obs=rng.random((n, dim), np.float32), reward=rng.random(n, np.float32), done=(k == 1).astype(np.uint8),
                       nsteps=np.where(k == 1, 1, steps).astype(np.int32), kind=k, fin_return=rng.random(n, np.float32),
                       fin_length=rng.integers(1, 3, n).astype(np.int32), terminal_obs=rng.random((n, dim), np.float32)) for k in kinds]


@pytest.mark.parametrize("n", [3, 1])
def test_auto_reset_rules_on_a_scripted_loop(models, n):
    """What step() promises with auto_reset=True, without the device: done = done | truncated, the episode infos, the step counts,
    goal points read back only after a reset, and the reference's scalar shapes with one env."""
    m = models["cfg2"]
    sim = EpisodeStandIn(m, n)
    env = VecHSREnv(model=m, n_envs=n, sim=sim, goals=[GoalSpec("block0", Box(low=[-.1, -.2, .422], high=[.1, .2, .422]), .05)],
                    steps_per_action=20, auto_reset=True, max_episode_steps=2)
    records = scripted_records(n, m.nq + m.nv)
    env._loop = ScriptedLoop(sim, records)
    sim.move_goal([.01, .02, .422])
    env.reset()
    assert np.array_equal(env._goal_points, np.tile(np.float32([.01, .02, .422]), (n, 1))) and not env._time_steps.any()
    sq = (lambda x: x[0]) if n == 1 else (lambda x: x)
    count, points = np.zeros(n, np.int64), env._goal_points.copy()
    for k, r in enumerate(records):
        sim.move_goal([.03 + .01 * k, 0, .422])                 # what the device would have drawn for the envs it reset
        obs, rew, done, info = env.step(np.zeros((n, m.nu)))
        assert np.array_equal(obs, sq(r.obs)) and np.array_equal(rew, sq(r.reward))
        assert np.array_equal(done, sq(r.kind != 0))
        assert np.array_equal(info["TimeLimit.truncated"], sq(r.kind == 2))
        assert np.array_equal(info["episode"]["r"], sq(r.fin_return)) and np.array_equal(info["episode"]["l"], sq(r.fin_length))
        assert np.array_equal(info["terminal_observation"], sq(r.terminal_obs))
        count = np.where(r.kind != 0, 0, count + 1)
        assert np.array_equal(env._time_steps, count)
        if (r.kind != 0).any():
            points = np.tile(np.float32([.03 + .01 * k, 0, .422]), (n, 1))
        assert np.array_equal(env._goal_points, points) and np.array_equal(env.goals[0].b, sq(points))
        if n == 1:
            assert obs.shape == (m.nq + m.nv,) and type(rew) is float and type(done) is bool
            assert type(info["TimeLimit.truncated"]) is bool and type(info["episode"]["r"]) is float and type(info["episode"]["l"]) is int
    assert np.array_equal(points[0], np.float32([.05, 0, .422]))       # the first record resets nobody, the other two do


def test_auto_reset_tells_the_recorder_each_step_then_each_reset(models, tmp_path):
    """record=True with auto_reset=True: per step one after_step with what the step latched, then one on_reset with the envs whose
    episode ended; the video counts its episodes by them."""
    import json
    from test_record_host import FakeCaptureSim

    class Sim(FakeCaptureSim):
        set_episodes = reset_sampled = lambda self, arg=None: None

        def body_xpos(self, body_id):
            return np.zeros((self.n, 3), np.float32)

    m, n = models["cfg2"], 3
    sim = Sim(m, n)
    env = VecHSREnv(model=m, n_envs=n, sim=sim, goals=[GoalSpec("block0", np.array([.4, 0, .422]), .05)], steps_per_action=20,
                    auto_reset=True, max_episode_steps=2, record=True, record_path=tmp_path, record_size=(8, 6), record_camera=object())
    records = scripted_records(n, m.nq + m.nv)
    env._loop = ScriptedLoop(sim, records)
    calls = []
    for name in ("after_step", "on_reset"):
        def spy(*args, _name=name, _call=getattr(env._recorder, name)):
            calls.append((_name,) + tuple(np.array(a) for a in args))
            return _call(*args)
        setattr(env._recorder, name, spy)
    env.reset()
    assert [c[0] for c in calls] == ["on_reset"] and calls[0][1].all() and not calls[0][2].any()
    for r in records:
        del calls[:]
        env.step(np.zeros((n, m.nu)))
        assert [c[0] for c in calls] == ["after_step", "on_reset"]
        assert np.array_equal(calls[0][1], r.done.astype(bool)) and np.array_equal(calls[0][2], r.nsteps)
        assert np.array_equal(calls[1][1], r.kind != 0) and calls[1][2].all()
    env.close()
    frames = json.loads((tmp_path / "env0.meta.json").read_text())["frames"]      # env 0: goes on, done (1 substep, 50 tail frames), out of time
    assert [(f["step"], f["episode"], f["tail"]) for f in frames] == [(0, 0, False)] + [(1, 0, False)] + [(1, 0, True)] * 50 + [(2, 1, False)]
