"""Recording without a GPU: the YUV4MPEG2 writer (hsr_env_amd/record.py), VecHSREnv's record arguments, and the frame bookkeeping of
a recording env (frames per step, the 50 trailing frames after done, episodes across resets), driven by a fake simulator that stands
in for BatchSim's capture calls."""
import json
from pathlib import Path

import numpy as np
import pytest

from hsr_env_amd import record as rec
from hsr_env_amd.env import VecHSREnv


# ------------------------------------------------------------------ the Y4M writer
def test_y4m_header_and_frame_size(tmp_path):
    v = rec.VideoRecorder(tmp_path / "a.y4m", 6, 4)
    for k in range(3):
        v.capture_frame(np.full((4, 6, 3), 10 * k, np.uint8), {"i": k})
    v.close()
    data = (tmp_path / "a.y4m").read_bytes()
    header = data[:data.index(b"\n")].decode().split()
    assert header[0] == "YUV4MPEG2" and "W6" in header and "H4" in header and "F30:1" in header and "C444" in header
    assert "XCOLORRANGE=FULL" in header
    assert len(data) == len(" ".join(header)) + 1 + 3 * (len(b"FRAME\n") + 3 * 6 * 4)
    meta = json.loads((tmp_path / "a.meta.json").read_text())
    assert meta["fps"] == 30 and [f["i"] for f in meta["frames"]] == [0, 1, 2]
    assert v.closed
    v.close()                                 # closing twice is harmless


def test_y4m_rejects_wrong_frames(tmp_path):
    v = rec.VideoRecorder(tmp_path / "b.y4m", 4, 4)
    with pytest.raises(ValueError):
        v.capture_frame(np.zeros((4, 5, 3), np.uint8))
    with pytest.raises(ValueError):
        v.capture_frame(np.zeros((4, 4, 3), np.float32))
    v.close()


@pytest.mark.parametrize("rgb,yuv", [((0, 0, 0), (0, 128, 128)), ((255, 255, 255), (255, 128, 128)),
                                     ((255, 0, 0), (76, 85, 255)), ((0, 255, 0), (150, 44, 21)), ((0, 0, 255), (29, 255, 107))])
def test_pure_colours_have_the_bt601_full_range_values(rgb, yuv):
    assert tuple(rec.rgb_to_yuv(np.array(rgb, np.uint8))) == yuv


def test_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (5, 8, 12, 3), dtype=np.uint8)
    v = rec.VideoRecorder(tmp_path / "c.y4m", 12, 8)
    for f in frames:
        v.capture_frame(f)
    v.close()
    hdr, yuv = rec.read_y4m(tmp_path / "c.y4m")
    assert hdr["W"] == "12" and hdr["H"] == "8" and yuv.shape == (5, 8, 12, 3)
    np.testing.assert_array_equal(yuv, rec.rgb_to_yuv(frames))
    back = rec.yuv_to_rgb(yuv).astype(int)
    assert np.abs(back - frames).max() <= 2


# ------------------------------------------------------------------ a fake simulator with BatchSim's capture surface
class FakeCaptureSim:
    """Env e runs `plan[e]` substeps per step (default: all of them; fewer = done early).  A frame's pixels encode (env, step, row)."""

    def __init__(self, model, n, plan=None):
        self.model, self.n = model, n
        self.nq, self.nv, self.nu = model.nq, model.nv, model.nu
        self.plan = plan or {}
        self.every, self.ids, self.steps, self.last = 0, [], 0, None

    def reset(self, mask=None, qpos0=None, mocap=None):
        pass

    def get_state(self):
        return np.zeros(self.n, np.float32), np.tile(self.model.qpos0, (self.n, 1)).astype(np.float32), np.zeros((self.n, self.nv), np.float32)

    def step(self, ctrl, n_substeps, goal_body=-1, geofence=0.0):
        ns = np.array([self.plan.get(e, lambda k: n_substeps)(self.steps) for e in range(self.n)], np.int32)
        done = ns < n_substeps
        self.last = (ns, n_substeps)
        self.steps += 1
        obs = np.zeros((self.n, self.nq + self.nv), np.float32)
        return obs, done.astype(np.float32), done, ns

    def set_capture(self, env_ids, every):
        self.ids, self.every = list(env_ids), every

    def capture_counts(self):
        ns, _ = self.last
        return np.array([0 if ns[e] == 0 else (ns[e] - 1) // self.every + 1 for e in self.ids], np.int32)

    def render_frames(self, width, height, camera=None, rgb=True, depth=False, segmentation=False, geom_rgba=None):
        _, nsub = self.last
        rows = (nsub - 1) // self.every + 2
        out = np.zeros((len(self.ids), rows, height, width, 3), np.uint8)
        for r, e in enumerate(self.ids):
            for k in range(rows):
                out[r, k] = (e, self.steps - 1, k)
        return out


def _env(models, tmp_path, n=4, plan=None, **kw):
    m = models["cfg1"]
    sim = FakeCaptureSim(m, n, plan)
    kw.setdefault("record", True)
    kw.setdefault("record_path", tmp_path)
    env = VecHSREnv(model=m, n_envs=n, sim=sim, goals=None, starts={}, steps_per_action=60, record_size=(8, 6), record_camera=object(), **kw)
    return env, sim


def test_record_arguments(models, tmp_path):
    env, sim = _env(models, tmp_path)
    assert sim.every == 20 and sim.ids == [0]                  # the reference's record_freq default; env 0 recorded by default
    env.close()
    env, sim = _env(models, tmp_path, record=False, record_freq=25, record_envs=[1, 3])
    assert sim.every == 25 and sim.ids == [1, 3]                # record_freq alone turns recording on (hsr/env.py:50)
    env.close()
    env, sim = _env(models, tmp_path, record=True, record_path=None)
    assert sim.every == 20 and env._recorder.path == Path("/tmp/training-video")       # hsr/env.py:55 (not closed: no file is written)
    env, sim = _env(models, tmp_path, record=False, record_path=None)
    assert sim.every == 0 and env._recorder is None
    env.close()
    with pytest.raises(NotImplementedError):
        _env(models, tmp_path, render=True)
    with pytest.raises(NotImplementedError):
        _env(models, tmp_path, record=False, record_path=None, render_freq=5)
    with pytest.raises(ValueError):
        _env(models, tmp_path, record_envs=[0, 0])
    with pytest.raises(ValueError):
        _env(models, tmp_path, record_envs=[4])


def test_record_without_sim_argument_does_not_raise(models, tmp_path, monkeypatch):
    """record=True used to raise NotImplementedError before the simulator was even built."""
    import hsr_env_amd.sim as hs
    monkeypatch.setattr(hs, "BatchSim", lambda model, n, device=0: FakeCaptureSim(model, n))
    env = VecHSREnv(model=models["cfg1"], n_envs=2, goals=None, starts={}, record=True, record_path=tmp_path, record_size=4,
                    record_camera=object())
    env.close()
    assert (tmp_path / "env0.y4m").exists() and (tmp_path / "env0.meta.json").exists()


def test_sharded_ranks_record_their_own_envs(models, tmp_path):
    m = models["cfg1"]
    ids = {}
    for rank in range(2):
        sim = FakeCaptureSim(m, 4)
        env = VecHSREnv(model=m, n_envs=4, sim=sim, env_offset=4 * rank, n_global=8, goals=None, starts={}, record=True,
                        record_envs=[1, 5, 6], record_path=tmp_path / f"r{rank}", record_size=4, record_camera=object())
        ids[rank] = sim.ids
        env.close()
    assert ids == {0: [1], 1: [1, 2]}
    assert sorted(p.name for p in (tmp_path / "r1").glob("*.y4m")) == ["env5.y4m", "env6.y4m"]


def test_frame_bookkeeping_across_steps_and_resets(models, tmp_path):
    # env 0 runs every step in full (60 substeps: frames at 0, 20, 40); env 3 stops after 1, 21 and 41 substeps in steps 0, 1, 2, then
    # runs in full
    plan = {3: lambda k: [1, 21, 41][k] if k < 3 else 60}
    env, sim = _env(models, tmp_path, plan=plan, record_envs=[0, 3], record_freq=20)
    env.reset()
    done = np.zeros(4, bool)
    for k in range(5):
        if done.any():
            env.reset(mask=done)
        _, _, done, _ = env.step(np.zeros((4, 2)))
    env.close()
    for g, per_step in ((0, [(3, False)] * 5), (3, [(1, True), (2, True), (3, True), (3, False), (3, False)])):
        meta = json.loads((tmp_path / f"env{g}.meta.json").read_text())["frames"]
        _, yuv = rec.read_y4m(tmp_path / f"env{g}.y4m")
        want = sum(rec.expected_frames(0 if n == 0 else 20 * (n - 1) + 1, 20, d) for n, d in per_step)
        assert len(meta) == len(yuv) == want
        rgb = rec.yuv_to_rgb(yuv)
        pos, episode = 0, 0
        for step, (n, d) in enumerate(per_step):
            for k in range(n):
                f = meta[pos]
                assert f == {"step": step, "episode": episode, "substep": 20 * k, "tail": False}
                assert np.abs(rgb[pos, 0, 0].astype(int) - [g, step, k]).max() <= 2
                pos += 1
            if d:
                for _ in range(50):
                    assert meta[pos]["tail"] and meta[pos]["step"] == step and meta[pos]["substep"] == 20 * (n - 1) + 1
                    assert np.abs(rgb[pos, 0, 0].astype(int) - [g, step, 3]).max() <= 2       # the final frame: the last row
                    pos += 1
                episode += 1
        assert pos == len(meta)


def test_expected_frames_formula():
    assert [rec.expected_frames(n, 20, False) for n in (0, 1, 20, 21, 40, 41, 300)] == [0, 1, 1, 2, 2, 3, 15]
    assert rec.expected_frames(21, 20, True) == 52
