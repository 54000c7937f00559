"""hsr_batch_render on the GPU: parity with the fp64 restatement (tests/render_ref.py) fed the batch's own link poses, analytic
scenes, independence from the batch, determinism, the physics left untouched, argument checks and the env surface."""
import time

import numpy as np
import pytest
import torch        # before the library: torch's HIP runtime must be the first one loaded into the process (as in test_rl.py)

import render_ref as rr
from hsr_env_amd import sim as hs
from hsr_env_amd.render import Camera, default_camera, default_palette, scene_bounds

pytestmark = pytest.mark.gpu

PARITY_MODELS = ("cfg1", "cfg2", "cfg3", "cfg4", "cupboard", "cfg3_setxml")


def _random_batch(m, n, seed, steps=2):
    rng = np.random.default_rng(seed)
    sim = hs.BatchSim(m, n)
    q0 = np.tile(m.qpos0, (n, 1)).astype(np.float32)
    qa, _ = m.scalar_joints()
    rg = m.dof_range.reshape(-1, 2)
    for a in qa:
        q0[:, a] += rng.uniform(-0.1, 0.1, n)
    for a in m.free_joint_qadrs():
        q0[:, a:a + 2] += rng.uniform(-0.05, 0.05, (n, 2))
    del rg
    sim.reset(qpos0=q0, mocap=np.tile([0.3, 0.0, 0.422], (n, 1)))
    lo, hi = m.act_ctrlrange[:, 0], m.act_ctrlrange[:, 1]
    acts = [rng.uniform(lo, hi, (n, m.nu)) for _ in range(steps)]
    for a in acts:
        sim.step(a, 20)
    return sim, acts


@pytest.mark.parametrize("cfg", PARITY_MODELS)
def test_parity_with_restatement(models, cfg):
    m = models[cfg]
    n, W = 16, 96
    sim, _ = _random_batch(m, n, seed=11)
    xpos, xmat = sim.get_field(hs.F_XPOS), sim.get_field(hs.F_XMAT)
    pal = default_palette(m)
    _, extent = scene_bounds(m)
    hulls = {}
    cams = [default_camera(m)]
    if m.block_body():
        cams.append(default_camera(m, m.body_id(m.block_body())))
    worst_amb = 0.0
    for cam in cams:
        rgb, depth, seg = sim.render(W, W, cam, rgb=True, depth=True, segmentation=True)
        for e in range(n):
            s_ref, d_ref, c_ref, amb, amb_rgb = rr.render_env(m, xpos[e], xmat[e], cam, W, W, pal, extent, hulls)
            worst_amb = max(worst_amb, amb.mean())
            bad = (seg[e] != s_ref) & ~amb
            assert not bad.any(), f"{cfg} env {e} track={cam.track_body}: {int(bad.sum())} pixels segment differently, e.g. " \
                                  f"{[(int(y), int(x), int(seg[e, y, x]), int(s_ref[y, x])) for y, x in zip(*np.nonzero(bad))][:4]}"
            same = (seg[e] == s_ref) & ~amb
            np.testing.assert_allclose(depth[e][same], d_ref[same], rtol=2e-5)
            ok = same & ~amb_rgb
            diff = np.abs(rgb[e].astype(int) - c_ref.astype(int))[ok]
            assert diff.max(initial=0) <= 1, f"{cfg} env {e}: rgb differs by {diff.max()}"
        assert (seg >= 0).mean() > 0.05, "the image is nearly empty"
    assert worst_amb < 0.01, f"{worst_amb:.3%} of an image is ambiguous"


def test_known_answers_static1(models):
    """static1: the robot welded to the world, block0 (a box) free.  The block placed far from everything, seen straight down."""
    m = models["static1"]
    sim = hs.BatchSim(m, 2)
    q = np.tile(m.qpos0, (2, 1)).astype(np.float32)
    a = m.free_joint_qadrs()[0]
    q[:, a:a + 7] = [5.0, 5.0, 1.0, 1, 0, 0, 0]
    sim.set_state(qpos=q, qvel=np.zeros((2, m.nv), np.float32))
    W = 64
    hx, hy, hz = m.geom_size[-1]
    cam = Camera(lookat=(5.0, 5.0, 1.0), distance=0.5, azimuth=90.0, elevation=-90.0, fovy=20.0, znear=0.01, zfar=50.0)
    rgb, depth, seg = sim.render(W, W, cam, rgb=True, depth=True, segmentation=True)
    d = 0.5 - hz
    c = ((np.arange(W) + 0.5) * (2.0 / W) - 1) * np.tan(np.deg2rad(10.0)) * d
    want = (np.abs(c)[:, None] <= hy) & (np.abs(c)[None, :] <= hx)
    np.testing.assert_array_equal(seg[0] == m.ngeom - 1, want)
    np.testing.assert_array_equal(seg[0][~want], -1)
    np.testing.assert_allclose(depth[0][want], d, rtol=2e-6)
    assert (depth[0][~want] == np.float32(50.0)).all() and (rgb[0][~want] == 0).all()
    assert (rgb[0][want][:, 1] >= 249).all() and (rgb[0][want][:, [0, 2]] == 0).all()
    # straight down onto the floor, away from everything else: depth = height everywhere
    cam = Camera(lookat=(1.7, -1.7, 0.0), distance=0.8, azimuth=90.0, elevation=-90.0, fovy=10.0, znear=0.01, zfar=50.0)
    depth, seg = sim.render(32, 32, cam, rgb=False, depth=True, segmentation=True)
    assert (seg == 0).all()
    np.testing.assert_allclose(depth, 0.8, rtol=2e-6)
    sim.close()


def test_known_answer_mesh_meshrest1(models):
    """meshrest1: block0 is a mesh hull; the ray straight down its origin meets the hull's top face at the hull's max z there."""
    m = models["meshrest1"]
    sim = hs.BatchSim(m, 1)
    q = m.qpos0[None].astype(np.float32).copy()
    a = m.free_joint_qadrs()[0]
    q[:, a:a + 7] = [-5.0, 5.0, 1.0, 1, 0, 0, 0]
    sim.set_state(qpos=q, qvel=np.zeros((1, m.nv), np.float32))
    g = m.ngeom - 1
    cam = Camera(lookat=(-5.0, 5.0, 1.0), distance=1.0, azimuth=90.0, elevation=-90.0, fovy=30.0, znear=0.01, zfar=50.0)
    W = 33
    depth, seg = sim.render(W, W, cam, rgb=False, depth=True, segmentation=True)
    geoms = rr.model_scene(m, sim.get_field(hs.F_XPOS)[0], sim.get_field(hs.F_XMAT)[0], default_palette(m))
    s_ref, d_ref, _, amb, _ = rr.render([geoms[g]], cam, W, W)
    assert seg[0, W // 2, W // 2] == g
    np.testing.assert_array_equal(seg[0][~amb], np.where(s_ref >= 0, g, -1)[~amb])
    np.testing.assert_allclose(depth[0][s_ref >= 0], d_ref[s_ref >= 0], rtol=2e-5)
    sim.close()


def test_independent_of_batch_and_deterministic(models):
    m = models["cfg3"]
    sim, _ = _random_batch(m, 64, seed=5)
    t, q, v = sim.get_state()
    e = 37
    cam = default_camera(m, m.body_id("block0"))
    r64 = sim.render(80, 48, cam, rgb=True, depth=True, segmentation=True)
    again = sim.render(80, 48, cam, rgb=True, depth=True, segmentation=True)
    for a, b in zip(r64, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    one = hs.BatchSim(m, 1)
    one.reset(mocap=np.array([[0.3, 0.0, 0.422]], np.float32))
    one.set_state(time=t[e:e + 1], qpos=q[e:e + 1], qvel=v[e:e + 1])
    # the same poses: the forward pass of set_state against those the step stored
    if np.array_equal(one.get_field(hs.F_XPOS)[0], sim.get_field(hs.F_XPOS)[e]) and \
            np.array_equal(one.get_field(hs.F_XMAT)[0], sim.get_field(hs.F_XMAT)[e]):
        r1 = one.render(80, 48, cam, rgb=True, depth=True, segmentation=True)
        for a, b in zip(r64, r1):
            assert np.array_equal(a[e:e + 1].view(np.uint8), b.view(np.uint8))
    # and unconditionally: a batch of 64 identical states renders 64 identical images, equal to a batch of 1 of that state
    big = hs.BatchSim(m, 64)
    big.reset(mocap=np.tile([0.3, 0.0, 0.422], (64, 1)).astype(np.float32))
    big.set_state(time=np.repeat(t[e:e + 1], 64), qpos=np.repeat(q[e:e + 1], 64, 0), qvel=np.repeat(v[e:e + 1], 64, 0))
    rb = big.render(80, 48, cam, rgb=True, depth=True, segmentation=True)
    r1 = one.render(80, 48, cam, rgb=True, depth=True, segmentation=True)
    for a, b in zip(rb, r1):
        assert np.array_equal(a.view(np.uint8), np.repeat(b, 64, 0).view(np.uint8))
    # the host path equals the device path
    import torch
    dev = torch.device("cuda", 0)
    t_rgb = torch.empty((64, 48, 80, 3), dtype=torch.uint8, device=dev)
    t_dep = torch.empty((64, 48, 80), dtype=torch.float32, device=dev)
    t_seg = torch.empty((64, 48, 80), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    sim.render_dev(80, 48, cam, rgb=t_rgb, depth=t_dep, segmentation=t_seg)
    sim.sync()
    for a, b in zip(r64, (t_rgb, t_dep, t_seg)):
        assert np.array_equal(a.view(np.uint8), b.cpu().numpy().view(np.uint8))
    # NULL palette = the Python default palette; another palette changes colours only
    assert np.array_equal(sim.render(80, 48, cam, geom_rgba=default_palette(m)), r64[0])
    pal = default_palette(m); pal[:, :3] = 1.0
    rgb2, seg2 = sim.render(80, 48, cam, rgb=True, segmentation=True, geom_rgba=pal)
    assert np.array_equal(seg2, r64[2]) and (rgb2[seg2 >= 0].min(1) == rgb2[seg2 >= 0].max(1)).all()
    for s in (sim, one, big):
        s.close()


@pytest.mark.parametrize("cfg,queue", [("cfg3", False), ("cfg4", True)])
def test_render_leaves_physics_untouched(models, cfg, queue):
    m = models[cfg]
    n = 64
    out = []
    for render in (False, True):
        rng = np.random.default_rng(3)
        sim = hs.BatchSim(m, n)
        if queue:
            sim.set_queue(1, 10)
        q0 = np.tile(m.qpos0, (n, 1)).astype(np.float32)
        q0[:, m.scalar_joints()[0]] += rng.uniform(-0.1, 0.1, (n, len(m.scalar_joints()[0])))
        sim.reset(qpos0=q0, mocap=np.tile([0.3, 0.0, 0.422], (n, 1)).astype(np.float32))
        goal = m.body_id(m.block_body())
        res = []
        for _ in range(3):
            if render:
                sim.render(64, 64, default_camera(m), rgb=True, depth=True, segmentation=True)
                sim.render(40, 24, default_camera(m, goal), rgb=True)
            res.append(sim.step(rng.uniform(m.act_ctrlrange[:, 0], m.act_ctrlrange[:, 1], (n, m.nu)), 30, goal, 0.05))
        res.append(sim.get_state())
        out.append(res)
        sim.close()
    for a, b in zip(out[0], out[1]):
        for x, y in zip(a, b):
            assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))


def test_argument_checks(models):
    m = models["cfg3"]
    sim = hs.BatchSim(m, 4)
    cam = default_camera(m)
    good = sim.render(32, 32, cam)
    bad_cams = [Camera(**{**cam.__dict__, k: v}) for k, v in
                (("fovy", 0.0), ("fovy", 180.0), ("znear", 0.0), ("zfar", cam.znear), ("distance", float("nan")),
                 ("lookat", (0.0, float("inf"), 0.0)), ("track_body", m.nbody), ("track_body", m.body_id("goal")))]
    for bc in bad_cams:
        with pytest.raises(AssertionError):
            sim.render(32, 32, bc)
    for w, h in ((0, 32), (32, 0), (4097, 8), (8, 4097)):
        with pytest.raises(AssertionError):
            sim.render(w, h, cam)
    assert np.array_equal(sim.render(32, 32, cam), good)
    sim.step(np.zeros((4, m.nu), np.float32), 5)
    sim.close()


def test_env_render_surface():
    from hsr_env_amd.env import VecHSREnv
    env = VecHSREnv(xml_file="cfg3", n_envs=8)
    env.reset()
    rgb = env.render("rgb_array", 64, 64)
    depth = env.render("depth_array", 64, 64)
    assert rgb.shape == (8, 64, 64, 3) and rgb.dtype == np.uint8
    assert depth.shape == (8, 64, 64) and depth.dtype == np.float32 and np.isfinite(depth).all()
    seg = env.sim.render(64, 64, rgb=False, segmentation=True)
    blk = [g for g, nm in enumerate(env.model.names["geom"]) if nm == "block0"][0]
    px = rgb[seg == blk].astype(int)
    assert len(px) > 0
    assert (px[:, 1] > px[:, 0]).all() and (px[:, 1] > px[:, 2]).all()
    env.close()
    one = VecHSREnv(xml_file="cfg3", n_envs=1)
    one.reset()
    assert one.render("rgb_array", 32, 16).shape == (16, 32, 3)
    one.close()


def test_render_at_size(models):
    import torch
    m = models["cfg3"]
    n = 8192
    sim = hs.BatchSim(m, n)
    sim.reset()
    dev = torch.device("cuda", 0)
    rgb = torch.empty((n, 64, 64, 3), dtype=torch.uint8, device=dev)
    depth = torch.empty((n, 64, 64), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    sim.render_dev(64, 64, None, rgb=rgb, depth=depth)
    sim.sync()
    t = time.perf_counter()
    sim.render_dev(64, 64, None, rgb=rgb, depth=depth)
    sim.sync()
    print(f"\n8192 envs x 64x64 rgb + depth: {1e3 * (time.perf_counter() - t):.2f} ms (host clock, one render)")
    assert torch.isfinite(depth).all()
    sim.close()
