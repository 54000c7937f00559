"""Rendering without a GPU: the library's hull face planes against scipy's, the fp64 restatement of the ray caster (tests/render_ref.py)
against analytic answers, the default camera and palette, and VecHSREnv.render's mode check."""
import ctypes as C

import numpy as np
import pytest

import render_ref as rr
from hsr_env_amd.render import Camera, default_camera, default_palette, scene_bounds

MESH_MODELS = ("cfg3", "cupboard", "meshrest1", "static1")
ALL_MODELS = ("cfg1", "cfg2", "cfg3", "cfg4", "cupboard", "cfg3_setxml", "nq18", "nv11", "nv23", "static1", "meshrest4", "meshrest1")


@pytest.fixture(scope="module")
def lib():
    from hsr_env_amd.build import build_lib
    L = C.CDLL(str(build_lib()))
    L.hsr_model_load.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)]
    L.hsr_model_destroy.argtypes = [C.c_void_p]
    L.hsr_model_hull_planes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    return L


@pytest.mark.parametrize("cfg", MESH_MODELS)
def test_hull_planes_match_scipy(lib, models, cfg):
    m = models[cfg]
    raw = m.to_bytes()
    h = C.c_void_p()
    assert lib.hsr_model_load(raw, len(raw), C.byref(h)) == 0
    try:
        mv = m.mesh_vert.reshape(-1, 3)
        nmesh = 0
        for g in range(m.ngeom):
            if m.geom_type[g] != rr.MESH:
                assert lib.hsr_model_hull_planes(h, g, None, 0) == -1
                continue
            nmesh += 1
            v = mv[m.geom_meshadr[g]:m.geom_meshadr[g] + m.geom_meshnum[g]]
            size = np.abs(v).max()
            n = lib.hsr_model_hull_planes(h, g, None, 0)
            assert n >= 4
            pl = np.zeros((n, 4), np.float32)
            assert lib.hsr_model_hull_planes(h, g, pl.ctypes.data, n) == n
            pl = pl.astype(np.float64)
            sd = v @ pl[:, :3].T - pl[:, 3]
            assert sd.max() <= 1e-6 * size, f"geom {g}: a vertex lies {sd.max():.3g} outside a plane"
            assert (np.abs(sd) <= 1e-6 * size).sum(0).min() >= 3, f"geom {g}: a plane touches fewer than 3 vertices"
            ref = rr.hull_planes(v)
            # scipy's facets merged with the test's tolerance
            merged = []
            for q in ref:
                if not any(np.abs(q[:3] - r[:3]).max() < 1e-5 and abs(q[3] - r[3]) <= 1e-6 * size for r in merged):
                    merged.append(q)
            merged = np.array(merged)
            close = (np.abs(pl[:, None, :3] - merged[None, :, :3]).max(2) < 1e-5) & (np.abs(pl[:, None, 3] - merged[None, :, 3]) <= 1e-6 * size)
            assert close.any(1).all(), f"geom {g}: {int((~close.any(1)).sum())} planes of the library have no scipy facet"
            assert close.any(0).all(), f"geom {g}: {int((~close.any(0)).sum())} scipy facets have no plane in the library"
        assert nmesh >= 1
    finally:
        lib.hsr_model_destroy(h)


def _down(lookat, dist, fovy=20.0, znear=0.01, zfar=50.0):
    return Camera(lookat=tuple(lookat), distance=dist, azimuth=90.0, elevation=-90.0, fovy=fovy, znear=znear, zfar=zfar)


def _px_centres(n, tan_half, depth):
    """world offsets of the pixel centres of one image axis at `depth` (left / top = negative)."""
    return ((np.arange(n) + 0.5) * (2.0 / n) - 1) * tan_half * depth


def test_restatement_floor_straight_down():
    floor = rr.Geom(0, rr.PLANE, np.array([2.0, 2.0, 2.0]), np.eye(3), np.zeros(3), np.array([.4, .3, .2, 1]))
    seg, depth, rgb, amb, _ = rr.render([floor], _down((0.3, -0.2, 0.0), 1.25), 32, 24)
    assert (seg == 0).all() and not amb.any()
    np.testing.assert_allclose(depth, 1.25, rtol=1e-12)
    # n = +z: shade 0.1 + 0.4 cos(angle of the pixel's ray to the vertical) + 0.5
    ty = np.tan(np.deg2rad(10.0))
    u, v = _px_centres(32, ty * 32 / 24, 1.0), _px_centres(24, ty, 1.0)
    cos = 1 / np.sqrt(1 + u[None, :] ** 2 + v[:, None] ** 2)
    want = np.floor(np.array([.4, .3, .2]) * (0.6 + 0.4 * cos)[..., None] * 255 + 0.5)
    np.testing.assert_array_equal(rgb, want.astype(np.uint8))


def test_restatement_box_face_on():
    hx, hy, hz = 0.05, 0.025, 0.017
    box = rr.Geom(3, rr.BOX, np.array([hx, hy, hz]), np.eye(3), np.array([0.0, 0.0, 1.0]), np.array([0, 1, 0, 1.0]))
    cam = _down((0.0, 0.0, 1.0), 0.5, fovy=20.0)
    W = H = 64
    seg, depth, rgb, amb, _ = rr.render([box], cam, W, H)
    d = 0.5 - hz
    ty = np.tan(np.deg2rad(10.0))
    xs, ys = _px_centres(W, ty, d), -_px_centres(H, ty, d)          # image right = +x, image up = +y
    want = (np.abs(ys)[:, None] <= hy) & (np.abs(xs)[None, :] <= hx)
    assert not amb[want].any()
    np.testing.assert_array_equal(seg >= 0, want)
    np.testing.assert_allclose(depth[want], d, rtol=1e-12)
    assert (depth[~want] == cam.zfar).all() and (rgb[~want] == 0).all()
    assert (rgb[want][:, [0, 2]] == 0).all() and (rgb[want][:, 1] >= 250).all()     # green, lit nearly head-on


def test_restatement_sphere_silhouette():
    r, dist = 0.1, 1.0
    sph = rr.Geom(5, rr.SPHERE, np.array([r, 0, 0]), np.eye(3), np.zeros(3), np.array([1, 1, 1, 1.0]))
    W = 101
    cam = _down((0, 0, 0), dist, fovy=30.0)
    seg, depth, _, _, _ = rr.render([sph], cam, W, W)
    # silhouette: the cone from the camera tangent to the sphere, half angle asin(r / dist); a pixel centre ray at (u, v, 1)
    ty = np.tan(np.deg2rad(15.0))
    c = _px_centres(W, ty, 1.0)
    ang = np.arctan(np.hypot(c[:, None], c[None, :]))
    np.testing.assert_array_equal(seg >= 0, ang <= np.arcsin(r / dist))
    assert abs(depth[W // 2, W // 2] - (dist - r)) < 1e-12


def test_restatement_cylinder_cap():
    rad, hl = 0.05, 0.2
    cyl = rr.Geom(7, rr.CYLINDER, np.array([rad, hl, 0]), np.eye(3), np.zeros(3), np.array([1, 1, 1, 1.0]))
    W = 64
    cam = _down((0, 0, 0), 1.0, fovy=10.0)
    seg, depth, rgb, _, _ = rr.render([cyl], cam, W, W)
    d = 1.0 - hl
    c = _px_centres(W, np.tan(np.deg2rad(5.0)), d)
    want = np.hypot(c[:, None], c[None, :]) <= rad
    np.testing.assert_array_equal(seg >= 0, want)
    np.testing.assert_allclose(depth[want], d, rtol=1e-12)
    assert (rgb[want] >= 252).all()            # cap normal +z toward a camera straight above


@pytest.mark.parametrize("cfg", ALL_MODELS)
def test_default_camera_and_palette(models, cfg):
    m = models[cfg]
    centre, extent = scene_bounds(m)
    assert np.isfinite(centre).all() and 0.1 < extent < 10
    cam = default_camera(m)
    a = cam.as_array()
    assert a.shape == (9,) and np.isfinite(a).all()
    assert cam.azimuth == 90 and cam.elevation == -45 and cam.fovy == 45 and cam.track_body == -1
    assert np.isclose(cam.distance, 1.5 * extent) and np.isclose(cam.znear, 0.01 * extent) and np.isclose(cam.zfar, 50 * extent)
    blk = m.block_body()
    if blk:
        assert default_camera(m, m.body_id(blk)).track_body == m.body_id(blk)
    pal = default_palette(m)
    assert pal.shape == (m.ngeom, 4) and pal.dtype == np.float32 and np.isfinite(pal).all()
    assert ((pal >= 0) & (pal <= 1)).all()
    for g, nm in enumerate(m.names["geom"]):
        if m.geom_type[g] == rr.PLANE:
            np.testing.assert_allclose(pal[g, :3], [.4, .3, .2], rtol=1e-6)
        if nm == "block":
            np.testing.assert_allclose(pal[g, :3], [.8, .1, .1], rtol=1e-6)
        if nm.split(":")[0] == "block0":
            np.testing.assert_array_equal(pal[g, :3], [0, 1, 0])
        if nm.split(":")[0] == "block1":
            np.testing.assert_array_equal(pal[g, :3], [0, 0, 1])
        if nm.startswith("hand_palm_link:") or nm.startswith("base_link:"):
            np.testing.assert_allclose(pal[g, :3], .33, rtol=1e-6)


def test_render_human_raises():
    from hsr_env_amd.env import VecHSREnv

    class _NoSim:
        def render(self, *a, **k):
            raise AssertionError("'human' must not reach the simulator")

    env = VecHSREnv.__new__(VecHSREnv)
    env.sim, env.n_envs = _NoSim(), 1
    with pytest.raises(NotImplementedError):
        env.render("human")
    with pytest.raises(ValueError):
        env.render("no_such_mode")
