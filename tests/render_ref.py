"""fp64 numpy restatement of the ray caster of hsr_batch_render (csrc/render.h) - test infrastructure, independent of the library's
hull planes (the hulls come from scipy.spatial.ConvexHull on the blob's vertices).

Same definitions as the kernel: MuJoCo free camera, ray dir = fwd + u right + v up (so the ray parameter is the depth along the camera
axis), pixel centres, row 0 at the top; nearest hit with znear <= depth <= zfar, ties to the lower geom id; planes front side only and
finite where size > 0; shading rgb = clamp(rgba (0.1 + 0.4 max(0, n.v) + 0.5 max(0, n.z)), 0, 1) rounded to 0..255.

Besides the image it returns two ambiguity masks where a single-precision caster may legitimately differ:
  amb     - segmentation / depth: the second-nearest hit lies within 1e-5 relative of the nearest, or some geom in front of the
            nearest hit is grazed (its entering interval, or the distance to its silhouette, within `tol` of empty), or the hit
            sits on a clip distance, or the nearest surface is seen at grazing incidence (|n.v| < 0.01, where a float ray
            direction moves the depth by ~1e-7 / |n.v|);
  amb_rgb - amb, or two faces tie for "entering" within `tol` (an edge: the normal, hence the shade, is either face's).
`tol` is 1e-5 x the scene extent: the kernel's fp32 ray / pose arithmetic at a few metres is good to ~1e-6 m.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from hsr_env_amd.compiler import quat_to_mat

PLANE, SPHERE, CYLINDER, BOX, MESH = 0, 2, 5, 6, 7


@dataclass
class Geom:
    gid: int
    type: int
    size: np.ndarray
    R: np.ndarray                 # geom -> world rotation
    p: np.ndarray                 # geom origin in the world
    rgba: np.ndarray
    planes: np.ndarray = field(default=None)   # mesh: [F, 4] (n, w), n.x <= w inside


def hull_planes(verts: np.ndarray, tol_rel: float = 1e-9) -> np.ndarray:
    """Face planes of the convex hull of `verts` (scipy), coplanar facets merged."""
    from scipy.spatial import ConvexHull
    eq = ConvexHull(verts).equations                       # n.x + off <= 0 inside
    size = np.abs(verts).max()
    out = []
    for n, off in zip(eq[:, :3], eq[:, 3]):
        n = n / np.linalg.norm(n)
        w = -off
        if not any(np.abs(q[:3] - n).sum() < 1e-7 and abs(q[3] - w) <= 1e-7 * size for q in out):
            out.append(np.array([*n, w]))
    return np.array(out)


def camera_frame(cam):
    """(fwd, right, up) of a render.Camera, as mjv_updateCamera forms them for a free camera."""
    az, el = np.deg2rad(cam.azimuth), np.deg2rad(cam.elevation)
    f = np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
    u = np.array([-np.sin(el) * np.cos(az), -np.sin(el) * np.sin(az), np.cos(el)])
    return f, np.cross(f, u), u


def model_scene(model, xpos, xmat, palette, hull_cache=None):
    """Geoms of one env placed by its link poses (xpos [nlink,3], xmat [nlink,3,3]; the world link is the identity)."""
    geoms = []
    mv = model.mesh_vert.reshape(-1, 3)
    hull_cache = {} if hull_cache is None else hull_cache
    for g in range(model.ngeom):
        l = model.geom_link[g]
        Rl, pl = (np.eye(3), np.zeros(3)) if l == 0 else (np.asarray(xmat[l], float).reshape(3, 3), np.asarray(xpos[l], float))
        Rg = quat_to_mat(model.geom_quat[g])
        planes = None
        if model.geom_type[g] == MESH:
            if g not in hull_cache:
                a = model.geom_meshadr[g]
                hull_cache[g] = hull_planes(mv[a:a + model.geom_meshnum[g]])
            planes = hull_cache[g]
        geoms.append(Geom(g, int(model.geom_type[g]), np.asarray(model.geom_size[g], float), Rl @ Rg, pl + Rl @ model.geom_pos[g],
                          np.asarray(palette[g], float), planes))
    return geoms


def _hit(g: Geom, o, d, tol):
    """Per ray (o [3] in the geom frame, d [P,3]): entering t, normal in the geom frame, signed margin (length; < 0 = miss) and the
    gap to the runner-up entering face (length; inf where there is none)."""
    P = d.shape[0]
    dn = np.linalg.norm(d, axis=1)
    inf = np.full(P, np.inf)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if g.type == PLANE:
            t0 = np.where(d[:, 2] < 0, -o[2] / d[:, 2], np.inf)
            hx, hy = o[0] + t0 * d[:, 0], o[1] + t0 * d[:, 1]
            mx = g.size[0] - np.abs(hx) if g.size[0] > 0 else inf
            my = g.size[1] - np.abs(hy) if g.size[1] > 0 else inf
            marg = np.where((o[2] > 0) & (d[:, 2] < 0), np.minimum(mx, my), -np.inf)
            n = np.tile([0.0, 0.0, 1.0], (P, 1))
            return t0, n, marg, inf
        if g.type == SPHERE:
            a = (d * d).sum(1)
            tc = -(d @ o) / a
            q = o + d * tc[:, None]
            qn = np.linalg.norm(q, axis=1)
            h2 = (g.size[0] ** 2 - qn ** 2) / a
            t0 = tc - np.sqrt(np.maximum(h2, 0))
            n = o + d * t0[:, None]
            return t0, n / np.linalg.norm(n, axis=1)[:, None], g.size[0] - qn, inf
        if g.type == CYLINDER:
            r, hl = g.size[0], g.size[1]
            a = d[:, 0] ** 2 + d[:, 1] ** 2
            tc = -(o[0] * d[:, 0] + o[1] * d[:, 1]) / a
            qx, qy = o[0] + tc * d[:, 0], o[1] + tc * d[:, 1]
            qn = np.hypot(qx, qy)
            sq = np.sqrt(np.maximum((r * r - qn * qn) / a, 0))
            s0, s1 = tc - sq, tc + sq
            za, zb = (-hl - o[2]) / d[:, 2], (hl - o[2]) / d[:, 2]
            c0, c1 = np.fmin(za, zb), np.fmax(za, zb)
            c0 = np.where(d[:, 2] == 0, np.where(abs(o[2]) <= hl, -np.inf, np.inf), c0)
            c1 = np.where(d[:, 2] == 0, np.where(abs(o[2]) <= hl, np.inf, -np.inf), c1)
            t0, t1 = np.maximum(s0, c0), np.minimum(s1, c1)
            side = s0 >= c0
            hp = o + d * t0[:, None]
            ns = np.stack([hp[:, 0], hp[:, 1], 0 * hp[:, 0]], 1)
            ns = ns / np.maximum(np.linalg.norm(ns, axis=1), 1e-300)[:, None]
            ncap = np.stack([0 * t0, 0 * t0, np.where(d[:, 2] > 0, -1.0, 1.0)], 1)
            n = np.where(side[:, None], ns, ncap)
            marg = np.minimum(r - qn, (t1 - t0) * dn)
            return t0, n, marg, np.abs(s0 - c0) * dn
        if g.type == BOX:
            nrm = np.concatenate([np.eye(3), -np.eye(3)])
            pl = np.concatenate([nrm, np.concatenate([g.size, g.size])[:, None]], 1)
        else:
            pl = g.planes
        den = d @ pl[:, :3].T                            # [P, F]
        num = pl[:, 3][None, :] - (pl[:, :3] @ o)[None, :]
        t = num / den
        ent = np.where(den < 0, t, -np.inf)
        lev = np.where(den > 0, t, np.inf)
        lev = np.where((den == 0) & (num < 0), -np.inf, lev)
        order = np.argsort(-ent, axis=1)
        k0 = order[:, 0]
        t0 = ent[np.arange(P), k0]
        t_2 = ent[np.arange(P), order[:, 1]] if pl.shape[0] > 1 else np.full(P, -np.inf)
        t1 = lev.min(1)
        n = pl[k0, :3]
        return t0, n, (t1 - t0) * dn, (t0 - t_2) * dn


def render(geoms, cam, width, height, track_point=None, extent=1.0):
    """-> (seg int32 [H,W], depth [H,W], rgb uint8 [H,W,3], amb bool [H,W], amb_rgb bool [H,W])."""
    f, r, u = camera_frame(cam)
    ty = np.tan(np.deg2rad(cam.fovy) / 2)
    tx = ty * width / height
    look = np.asarray(cam.lookat, float) + (0 if track_point is None else np.asarray(track_point, float))
    org = look - cam.distance * f
    px, py = np.meshgrid(np.arange(width), np.arange(height))
    U = ((px.ravel() + 0.5) * (2.0 / width) - 1) * tx
    V = (1 - (py.ravel() + 0.5) * (2.0 / height)) * ty
    D = f[None, :] + U[:, None] * r[None, :] + V[:, None] * u[None, :]
    P = D.shape[0]
    tol = 1e-5 * extent
    best = np.full(P, np.inf); second = np.full(P, np.inf)
    seg = np.full(P, -1, np.int32); nrm = np.zeros((P, 3)); col = np.zeros((P, 3)); tie = np.full(P, np.inf)
    grazes = []
    for g in geoms:
        o = g.R.T @ (org - g.p)
        d = D @ g.R
        t0, n, marg, gap = _hit(g, o, d, tol)
        ok = (marg >= 0) & (t0 >= cam.znear) & (t0 <= cam.zfar)
        grazes.append((t0, marg))
        better = ok & (t0 < best)
        second = np.where(better, best, np.where(ok, np.minimum(second, t0), second))
        best = np.where(better, t0, best)
        seg = np.where(better, g.gid, seg)
        nrm = np.where(better[:, None], n @ g.R.T, nrm)
        col = np.where(better[:, None], g.rgba[None, :3], col)
        tie = np.where(better, gap, tie)
    hit = seg >= 0
    depth = np.where(hit, best, cam.zfar)
    vdir = -D / np.linalg.norm(D, axis=1)[:, None]
    sh = 0.1 + 0.4 * np.maximum(0, (nrm * vdir).sum(1)) + 0.5 * np.maximum(0, nrm[:, 2])
    rgb = np.where(hit[:, None], np.floor(np.clip(col * sh[:, None], 0, 1) * 255 + 0.5), 0).astype(np.uint8)
    rel = 1e-5
    amb = hit & (second <= best * (1 + rel))
    amb |= hit & ((np.abs(best - cam.znear) <= rel * cam.znear) | (np.abs(best - cam.zfar) <= rel * cam.zfar))
    amb |= hit & (np.abs((nrm * vdir).sum(1)) < 1e-2)       # grazing incidence: the depth's condition number is 1 / |n.v|
    lim = np.where(hit, best * (1 + rel), cam.zfar * (1 + rel))
    for t0, marg in grazes:
        amb |= (np.abs(marg) < tol) & (t0 <= lim) & (t0 >= cam.znear * (1 - rel))
    amb_rgb = amb | (hit & (tie < tol))
    sh2 = lambda a: a.reshape(height, width)
    return sh2(seg), sh2(depth), rgb.reshape(height, width, 3), sh2(amb), sh2(amb_rgb)


def render_env(model, xpos, xmat, cam, width, height, palette, extent, hull_cache=None):
    """render() of one env of a batch from its link poses; a tracking camera looks at the tracked body's origin + lookat."""
    tp = None
    if cam.track_body >= 0:
        l = model.body_link[cam.track_body]
        Rl = np.eye(3) if l == 0 else np.asarray(xmat[l], float).reshape(3, 3)
        tp = (np.zeros(3) if l == 0 else np.asarray(xpos[l], float)) + Rl @ model.body_pos[cam.track_body]
    return render(model_scene(model, xpos, xmat, palette, hull_cache), cam, width, height, tp, extent)
