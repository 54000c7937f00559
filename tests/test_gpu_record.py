"""In-step frame capture and recording on the GPU (include/hsrsim.h: hsr_batch_set_capture, _capture_counts, _capture_poses,
_render_frames; hsr_env_amd/record.py): capture leaves the physics bit-identical in every mode of the persistent kernel and on the
per-substep chain; frame k holds the poses of substep k * every; the counts follow nsteps; both paths agree; the rendered frames are
the images hsr_batch_render draws from the same poses; the env and the control CLI write the videos."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch        # before the library: torch's HIP runtime must be the first one loaded into the process (as in test_rl.py)

from hsr_env_amd import sim as hs
from hsr_env_amd import record as rec
from hsr_env_amd.render import default_camera
from test_gpu_parity import random_states

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

N = 330
SUB = 60
EVERY = 7
# modes: (model, batch setup); the goal below makes some envs finish early
MODES = {
    "persistent": ("cfg3", lambda s: s.set_queue(0, 0)),
    "queue": ("cfg4", lambda s: s.set_queue(1, 7)),
    "solo": ("cfg3", lambda s: (s.set_solo(N, 0.01), s.set_queue(1, 10))),
    "chain_graph": ("cfg3", lambda s: (s.set_persistent(False), s.set_graph(True))),
    "chain_plain": ("cfg3", lambda s: (s.set_persistent(False), s.set_graph(False))),
}


def _case(m, seed=61):
    rng = np.random.default_rng(seed)
    q, v, ctrl = random_states(m, N, rng)
    goal = np.tile([0.0, 0.0, 0.422], (N, 1)).astype(np.float32)
    ids = np.sort(rng.choice(N, 40, replace=False)).astype(np.int32)
    return q, v, ctrl, goal, ids


def _batch(m, mode, q, v, goal):
    sim = hs.BatchSim(m, N)
    MODES[mode][1](sim)
    sim.set_mocap(goal)
    sim.set_state(np.zeros(N), q, v)
    return sim


def _fresh_poses(m, mode, q, v, ctrl, goal, nsub):
    """xpos / xmat of a fresh, identical batch after one env-step of nsub substeps."""
    sim = _batch(m, mode, q, v, goal)
    sim.step(ctrl, nsub, m.body_id(m.block_body()), 0.1)
    out = sim.get_field(hs.F_XPOS), sim.get_field(hs.F_XMAT).reshape(N, m.nlink, 3, 3)
    sim.close()
    return out


@pytest.mark.parametrize("mode", list(MODES))
def test_capture_leaves_the_physics_bit_identical(models, mode):
    m = models[MODES[mode][0]]
    q, v, ctrl, goal, ids = _case(m)
    res = []
    for cap in (False, True):
        sim = _batch(m, mode, q, v, goal)
        if cap:
            sim.set_capture(ids, EVERY)
        out = []
        for k in range(3):
            obs, rew, done, ns = sim.step(ctrl, SUB, m.body_id(m.block_body()), 0.1)
            t, qq, vv = sim.get_state()
            out += [obs, rew, done, ns, t, qq, vv, sim.get_field(hs.F_XPOS), sim.get_field(hs.F_XMAT)]
            if cap:
                assert (sim.capture_counts() > 0).all()
        assert not sim.bad_state()[1]
        res.append(out)
        sim.close()
    assert 0 < res[0][2].sum() < N, "the case needs early exits and full env-steps"
    for a, b in zip(*res):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("mode", list(MODES))
def test_frames_hold_the_poses_of_their_substep(models, mode):
    """Frame k = the poses after a fresh batch ran k * every + 1 substeps (bit for bit where both runs take the same kernel path; the
    work queue and the solo servers do not run for one-round env-steps, so there a tolerance applies); the final
    frame = F_XPOS / F_XMAT after the step; counts = (nsteps - 1) // every + 1; rows past a slot's count stay NaN."""
    m = models[MODES[mode][0]]
    q, v, ctrl, goal, ids = _case(m)
    every = 20
    sim = _batch(m, mode, q, v, goal)
    sim.set_capture(ids, every)
    _, _, done, ns = sim.step(ctrl, SUB, m.body_id(m.block_body()), 0.1)
    counts = sim.capture_counts()
    xpos, xmat = sim.capture_poses()
    rows = (SUB - 1) // every + 2
    assert sim.capture_rows() == rows and xpos.shape == (len(ids), rows, m.nlink, 3) and xmat.shape == (len(ids), rows, m.nlink, 3, 3)
    np.testing.assert_array_equal(counts, np.where(ns[ids] > 0, (ns[ids] - 1) // every + 1, 0))
    assert done[ids].any() and (~done[ids]).any(), "the recorded envs need early exits and full env-steps"
    assert (counts < rows - 1).any(), "some slot must leave rows unwritten"
    np.testing.assert_array_equal(xpos[:, -1], sim.get_field(hs.F_XPOS)[ids])
    np.testing.assert_array_equal(xmat[:, -1], sim.get_field(hs.F_XMAT).reshape(N, m.nlink, 3, 3)[ids])
    for r in range(len(ids)):
        for k in range(counts[r], rows - 1):
            assert np.isnan(xpos[r, k]).all() and np.isnan(xmat[r, k]).all(), (r, k)
    # a new setting poisons the buffer again: the rows the next step does not write are NaN
    sim.set_capture(ids, every)
    _, _, _, ns2 = sim.step(ctrl, SUB, m.body_id(m.block_body()), 0.1)
    x2, _ = sim.capture_poses()
    c2 = sim.capture_counts()
    np.testing.assert_array_equal(c2, np.where(ns2[ids] > 0, (ns2[ids] - 1) // every + 1, 0))
    for r in range(len(ids)):
        assert np.isnan(x2[r, c2[r]:rows - 1]).all() and np.isfinite(x2[r, :c2[r]]).all() and np.isfinite(x2[r, -1]).all()
    sim.close()
    exact = mode in ("persistent", "chain_graph", "chain_plain")
    errs = []
    for k in range(rows - 1):
        have = counts > k
        fp, fm = _fresh_poses(m, mode, q, v, ctrl, goal, k * every + 1)
        if exact:
            np.testing.assert_array_equal(xpos[have, k], fp[ids[have]])
            np.testing.assert_array_equal(xmat[have, k], fm[ids[have]])
        else:
            errs.append(np.abs(xpos[have, k] - fp[ids[have]]).max(axis=(1, 2)))
            errs.append(np.abs(xmat[have, k] - fm[ids[have]]).max(axis=(1, 2, 3)))
    if not exact:
        err = np.concatenate(errs)
        if mode == "queue":          # the persistent-vs-chain tolerance (tests/test_gpu_parity.py)
            assert (err < 2e-5).mean() >= 0.95 and np.median(err) < 1e-6, np.sort(err)[-5:]
        else:                        # servers sum in another order: the tolerance of tests/test_gpu_hotpath.py::test_solo_servers_follow_the_plain_run
            assert (err < 2e-3).mean() >= 0.9 and np.median(err) < 1e-5, np.sort(err)[-5:]


def test_persistent_and_chain_frames_agree(models):
    """The persistent kernel and the per-substep chain capture the same frames within the persistent-vs-chain tolerance
    (tests/test_gpu_parity.py::test_persistent_kernel_matches_per_substep_kernels)."""
    m = models["cfg3"]
    q, v, ctrl, goal, ids = _case(m, seed=62)
    res = []
    for mode in ("persistent", "chain_graph"):
        sim = _batch(m, mode, q, v, goal)
        sim.set_capture(ids, EVERY)
        _, _, _, ns = sim.step(ctrl, SUB, m.body_id(m.block_body()), 0.1)
        res.append((ns[ids], sim.capture_counts(), *sim.capture_poses()))
        sim.close()
    (na, ca, pa, ma), (nb, cb, pb, mb) = res
    same = na == nb
    assert same.mean() >= 0.95
    np.testing.assert_array_equal(ca[same], cb[same])
    err = []
    for r in np.flatnonzero(same):
        for k in list(range(ca[r])) + [-1]:
            err.append(max(np.abs(pa[r, k] - pb[r, k]).max(), np.abs(ma[r, k] - mb[r, k]).max()))
    err = np.array(err)
    assert (err < 2e-5).mean() >= 0.95 and np.median(err) < 1e-6, np.sort(err)[-5:]


@pytest.mark.parametrize("track", [False, True])
def test_rendered_frames_equal_render_of_the_same_poses(models, track):
    m = models["cfg3"]
    q, v, ctrl, goal, ids = _case(m, seed=63)
    ids = ids[:8]
    every, W, H = 20, 48, 40
    cam = default_camera(m, m.body_id(m.block_body()) if track else -1)
    sim = _batch(m, "persistent", q, v, goal)
    sim.set_capture(ids, every)
    sim.step(ctrl, SUB, m.body_id(m.block_body()), 0.1)
    counts = sim.capture_counts()
    rgb, dep, seg = sim.render_frames(W, H, cam, rgb=True, depth=True, segmentation=True)
    rows = sim.capture_rows()
    assert rgb.shape == (len(ids), rows, H, W, 3) and dep.shape == seg.shape == (len(ids), rows, H, W)
    r0, d0, s0 = sim.render(W, H, cam, rgb=True, depth=True, segmentation=True)            # the final frame: the batch's own poses
    np.testing.assert_array_equal(rgb[:, -1], r0[ids]); np.testing.assert_array_equal(dep[:, -1], d0[ids]); np.testing.assert_array_equal(seg[:, -1], s0[ids])
    for r in range(len(ids)):              # rows past a slot's count are not written (render_frames fills them with 0 / NaN / -2)
        assert (seg[r, counts[r]:rows - 1] == -2).all() and np.isnan(dep[r, counts[r]:rows - 1]).all()
    sim.close()
    for k in range(rows - 1):
        have = np.flatnonzero(counts > k)
        f = _batch(m, "persistent", q, v, goal)
        f.step(ctrl, k * every + 1, m.body_id(m.block_body()), 0.1)
        r1, d1, s1 = f.render(W, H, cam, rgb=True, depth=True, segmentation=True)
        f.close()
        np.testing.assert_array_equal(rgb[have, k], r1[ids[have]])
        np.testing.assert_array_equal(dep[have, k], d1[ids[have]])
        np.testing.assert_array_equal(seg[have, k], s1[ids[have]])
    assert (seg[:, :-1] >= 0).any(), "the frames must show geoms"


def test_capture_arguments(models):
    m = models["cfg2"]
    sim = hs.BatchSim(m, 16)
    with pytest.raises(AssertionError):
        sim.capture_counts()                                   # no capture yet
    for ids, every in (([0], -1), ([16], 5), ([-1], 5), ([2, 2], 5), (list(range(16)) * 70, 5), ([], 5)):
        with pytest.raises(AssertionError):
            sim.set_capture(ids, every)
    sim.set_capture([3], 5)
    with pytest.raises(AssertionError):
        sim.render_frames(8, 8)                                # no step since set_capture
    sim.step(np.zeros((16, m.nu)), 12)
    assert sim.capture_rows() == 4 and sim.capture_counts().tolist() == [3]
    with pytest.raises(AssertionError):
        sim.render_frames(0, 8)
    sim.set_capture([], 0)
    with pytest.raises(AssertionError):
        sim.capture_counts()
    sim.close()


def test_env_records_videos(models, tmp_path):
    """VecHSREnv(record=True, record_freq=25, record_envs=[0, 3]) over steps with resets: two videos whose frame counts match the meta
    and the formula (50 trailing frames after done) and whose decoded frames are render_frames' images within YUV rounding."""
    from hsr_env_amd.env import GoalSpec, VecHSREnv
    m = models["cfg3"]
    n, S, size = 8, 60, 64
    cam = default_camera(m)
    env = VecHSREnv(model=m, n_envs=n, goals=[GoalSpec(m.block_body(), np.array([0.0, 0.0, 0.422]), 0.05)], starts={},
                    steps_per_action=S, record=True, record_freq=25, record_envs=[0, 3], record_path=tmp_path, record_size=size,
                    record_camera=cam)
    ba = m.free_joint_qadrs()[0]
    env.reset()
    expect = {0: [], 3: []}
    done = np.zeros(n, bool)
    saw_done = {0: False, 3: False}
    for k in range(5):
        if done.any():
            env.reset(mask=done)
        t, qq, vv = env.sim.get_state()
        # env 0 starts on the goal in even steps, env 3 in steps 0 and 3 (they finish at their first substep); elsewhere far from it
        for e, on in ((0, k % 2 == 0), (3, k % 3 == 0)):
            qq[e, ba:ba + 3] = [0.0, 0.0, 0.422] if on else [0.1, 0.2, 0.422]
        env.set_state(qq, vv)
        _, _, done, info = env.step(np.zeros((n, m.nu)))
        ns = info["substeps"]
        counts = env.sim.capture_counts()
        frames = env.sim.render_frames(size, size, cam)
        for r, e in enumerate((0, 3)):
            assert counts[r] == (ns[e] - 1) // 25 + 1
            expect[e] += [frames[r, j] for j in range(counts[r])] + ([frames[r, -1]] * 50 if done[e] else [])
            saw_done[e] |= bool(done[e])
        assert done[0] == (k % 2 == 0) and done[3] == (k % 3 == 0)
    env.close()
    assert saw_done == {0: True, 3: True}
    assert sorted(p.name for p in tmp_path.glob("*.y4m")) == ["env0.y4m", "env3.y4m"]
    for e in (0, 3):
        meta = json.loads((tmp_path / f"env{e}.meta.json").read_text())
        hdr, yuv = rec.read_y4m(tmp_path / f"env{e}.y4m")
        assert len(meta["frames"]) == len(yuv) == len(expect[e])
        assert sum(f["tail"] for f in meta["frames"]) == 50 * sum(1 for k in range(5) if (k % 2 == 0 if e == 0 else k % 3 == 0))
        assert [f["step"] for f in meta["frames"]] == sorted(f["step"] for f in meta["frames"])
        assert np.abs(rec.yuv_to_rgb(yuv).astype(int) - np.stack(expect[e]).astype(int)).max() <= 2


def test_control_cli_records(tmp_path):
    out = tmp_path / "videos"
    cmd = [sys.executable, "-m", "hsr_env_amd.control", "--steps-per-action", "30", "--geofence", ".05",
           "--goal-space", "(-.1,.1)(-.2,.2)(.422,.422)", "--block-space", "(-.1,.1)(-.2,.2)(.422,.422)(-3.14,3.14)",
           "--n-blocks", "1", "--n-envs", "4", "--env-steps", "3", "--record", "--record-freq", "10", "--record-path", str(out)]
    from hsr_env_amd.compiler import ALL_DOFS
    for d in ALL_DOFS:                                         # cfg3: every dof, one block
        cmd += ["--use-dof", d]
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    meta = json.loads((out / "env0.meta.json").read_text())
    hdr, yuv = rec.read_y4m(out / "env0.y4m")
    assert hdr["W"] == "500" and hdr["H"] == "500"
    steps = {f["step"] for f in meta["frames"]}
    assert len(yuv) == len(meta["frames"]) >= 3 and steps == {0, 1, 2}
