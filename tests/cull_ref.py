"""Inputs and reference of tests/test_gpu_culls.py: pairs of the committed models' shapes at grazing distance, placed without any product code, and what
exact geometry says about each.

Placement: for a unit direction u the second shape is put so that its support point along -u lies g along u from the first shape's support point along u.
Poses are rounded to fp32 first (they are the kernels' inputs); everything below is evaluated in fp64 on the rounded values:
  gap   = (sB - sA) . u, the separation along u.  gap > 0: the plane orthogonal to u separates the shapes, their distance is at least gap,
  dup   = |sB - sA|, the distance of two points of the shapes: their distance is at most dup,
  depth = geom_checks.exact_penetration of the two vertex sets where gap <= 0 (nan elsewhere).  A cylinder is represented by an inscribed prism with a vertex
          at its support point - a subset of the cylinder, so a depth it proves is a depth the cylinder has; its support point itself is analytic.
A shape is the image of its local vertices under the ROUNDED matrix (no longer exactly orthonormal: the half extents change by 6e-8 of their length, far
below the 2e-6 from which anything is asserted).
Bounding boxes: bc / bh from geom_aabb as load_geom_v (csrc/collide.h) forms them, in fp32.

The harness lays 64 rows into a wave and switches lane % 4 == 3 of every odd wave off: layout() puts filler rows there and remembers where the real ones went.
emulate() restates the cull functions in numpy fp32 - for the CPU self-test of this module only (tests/test_cull_bounds.py does not use it; the GPU test
reads the device's words, never the emulation)."""
import functools
import re
from pathlib import Path

import numpy as np

import geom_checks as gc
from hsr_env_amd import model as hm

ROOT = Path(__file__).resolve().parent.parent
HARNESS = ROOT / "tools" / "micro" / "culls.hip"
IN_W, OUT_W = 64, 16
SENTINEL = 0xDEADBEEF
SKIN = float(re.search(r"#define\s+HSR_SKIN\s+([0-9.eE+-]+)f", (ROOT / "hsr_env_amd" / "csrc" / "solve_g.h").read_text()).group(1))
DEMAND = 2e-6                      # the depth from which tests/test_gpu_geometry.py demands a contact
GAPS = [s * v for v in (2e-6, 1e-5, 1e-4, 1e-3) for s in (-1, 1)] + [SKIN - 2e-6, SKIN + 2e-6, SKIN - 1e-4, SKIN + 1e-4, 0.5 * SKIN, 2 * SKIN]
CTRL_BH, CTRL_RB = 1e-4, 0.01      # the negative control: every bh smaller by this much, every radius by this fraction
PRISM = 180                        # sides of the prism inscribed in a cylinder
MODELS = ("cfg1", "cfg2", "cfg3", "cfg4", "cupboard", "cfg3_setxml", "nq18", "nv11", "nv23", "static1", "meshrest4", "meshrest1")


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


class Shape:
    """a geom of a committed model with the tables the device holds of it (fp32 values, kept in fp64)"""

    def __init__(self, m, name):
        g = m.names["geom"].index(name)
        self.name, self.type = name, int(m.geom_type[g])
        self.size, self.aabb, self.rb = f32(m.geom_size[g]), f32(m.geom_aabb[g]), float(f32(m.geom_rbound[g]))
        self.nvert = int(m.geom_meshnum[g])
        a = int(m.geom_meshadr[g])
        self.verts = f32(m.mesh_vert[a:a + self.nvert]) if self.type == hm.GEOM_MESH else None
        if self.type == hm.GEOM_BOX:
            self.verts = np.array([[sx * self.size[0], sy * self.size[1], sz * self.size[2]] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
        self.kind = {hm.GEOM_PLANE: "plane", hm.GEOM_BOX: "box", hm.GEOM_MESH: "hull", hm.GEOM_CYLINDER: "cyl"}[self.type]

    def support_local(self, d):
        """the point of the shape farthest along d, in the geom frame"""
        if self.type == hm.GEOM_CYLINDER:
            r = np.hypot(d[0], d[1])
            xy = self.size[0] * d[:2] / r if r > 1e-300 else np.zeros(2)
            return np.array([xy[0], xy[1], self.size[1] if d[2] > 0 else -self.size[1]])
        return self.verts[int(np.argmax(self.verts @ d))]

    def local_vertices(self, d):
        """vertices whose hull is the shape - the cylinder: the inscribed prism with one edge through support_local(d)"""
        if self.type != hm.GEOM_CYLINDER:
            return self.verts
        ang = np.arctan2(d[1], d[0]) + np.linspace(0, 2 * np.pi, PRISM, endpoint=False)
        ring = self.size[0] * np.stack([np.cos(ang), np.sin(ang)], 1)
        return np.concatenate([np.c_[ring, np.full(PRISM, self.size[1])], np.c_[ring, np.full(PRISM, -self.size[1])]])


@functools.lru_cache(maxsize=None)
def shapes():
    c3, cb = hm.load_config("cfg3"), hm.load_config("cupboard")
    S = {"block": Shape(c3, "block0"), "table": Shape(c3, "geom1"), "plane": Shape(c3, "floor"), "cyl": Shape(c3, "geom30"),
         "wrist": Shape(c3, "wrist_roll_link:wrist_roll"), "palm": Shape(c3, "hand_palm_link:palm"),
         "lprox": Shape(c3, "hand_l_spring_proximal_link:l_proximal"), "ldist": Shape(c3, "hand_l_distal_link:l_distal"),
         "rdist": Shape(c3, "hand_r_distal_link:r_distal"), "cblock": Shape(cb, "block")}
    for i in (1, 4, 7, 11):
        S[f"pan{i}"] = Shape(cb, f"geom{i}")
    return S


# (first, second, replicates of the whole (u, orientation, gap) grid)
PAIRINGS = [("table", "block", 2), ("pan1", "cblock", 1), ("pan4", "cblock", 1), ("pan7", "cblock", 1), ("pan11", "cblock", 1), ("block", "block", 1),
            ("wrist", "block", 1), ("ldist", "block", 1), ("palm", "cblock", 1), ("block", "lprox", 1),
            ("ldist", "rdist", 1), ("wrist", "palm", 1),
            ("cyl", "block", 1), ("cyl", "ldist", 1),
            ("plane", "block", 1), ("plane", "ldist", 1), ("plane", "wrist", 1), ("plane", "cyl", 1)]


def rot(axis, ang):
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def second_orientation(rng, R1, okind):
    """0 random, 1 identical, 2 a 90 degree axis permutation, 3 / 4 the last two turned by 1e-8 .. 1e-3 rad: near-parallel edge axes"""
    if okind == 0:
        return gc.quat2mat(gc.random_quat(rng))
    R = R1.copy()
    if okind in (2, 4):
        R = R @ rot(np.eye(3)[rng.integers(3)], np.pi / 2 * rng.choice([-1, 1]))
    if okind in (3, 4):
        R = R @ rot(rng.normal(size=3), float(np.exp(rng.uniform(np.log(1e-8), np.log(1e-3)))))
    return R


def direction(rng, R1, R2, ukind):
    """0 random, 1 a face normal of the first shape's box, 2 the cross product of one axis of each shape"""
    if ukind == 1:
        u = R1[:, rng.integers(3)]
    elif ukind == 2:
        for _ in range(20):
            u = np.cross(R1[:, rng.integers(3)], R2[:, rng.integers(3)])
            if np.linalg.norm(u) > 1e-12:
                break
    else:
        u = rng.normal(size=3)
    return u / np.linalg.norm(u) * rng.choice([-1, 1])


def geom_words(sh, pos, R):
    """pos[3] mat[9] size[3] bc[3] bh[3] as fp32, bc as load_geom_v forms it"""
    p32, R32, c32 = pos.astype(np.float32), R.astype(np.float32), sh.aabb[:3].astype(np.float32)
    bc = p32 + R32 @ c32
    return np.concatenate([p32, R32.reshape(9), sh.size.astype(np.float32), bc, sh.aabb[3:].astype(np.float32)])


def make_row(rng, A, B, ukind, okind, g):
    """-> (64 words, facts)"""
    pos1 = f32(rng.uniform(-2, 2, size=3))
    R1 = f32(gc.quat2mat(gc.random_quat(rng)) if not (A.type == hm.GEOM_PLANE and okind == 1) else np.eye(3))
    R2 = f32(second_orientation(rng, R1, okind))
    if A.type == hm.GEOM_PLANE:
        u = R1[:, 2] / np.linalg.norm(R1[:, 2])
        sA = pos1 + R1 @ np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), 0.0])          # any point of the plane
    else:
        u = direction(rng, R1, R2, ukind)
        sA = pos1 + R1 @ A.support_local(R1.T @ u)
    dl2 = R2.T @ (-u)
    sBl = B.support_local(dl2)
    pos2 = f32(sA + g * u - R2 @ sBl)
    sB = pos2 + R2 @ sBl
    gap, dup = float((sB - sA) @ u), float(np.linalg.norm(sB - sA))
    depth = np.nan
    if A.type == hm.GEOM_PLANE:
        gap = float((sB - pos1) @ u)          # signed distance of the second shape's lowest point
        dup, depth = abs(gap), -gap
    elif gap <= 0:
        va = pos1 + A.local_vertices(R1.T @ u) @ R1.T
        vb = pos2 + B.local_vertices(dl2) @ R2.T
        depth = gc.exact_penetration(va, vb)[0]
    w = np.zeros(IN_W, dtype=np.uint32)
    w[0:6] = [A.type, A.nvert, 0, B.type, B.nvert, 0]
    w[6:9] = [0, 1, hm.FN_PLANE_CONVEX if A.type == hm.GEOM_PLANE else hm.FN_CONVEX]
    fl = np.concatenate([geom_words(A, pos1, R1), geom_words(B, pos2, R2),
                         np.array([A.rb, B.rb, SKIN, B.rb if A.type == hm.GEOM_PLANE else np.float32(A.rb) + np.float32(B.rb)], dtype=np.float32)]).astype(np.float32)
    w[10:56] = fl.view(np.uint32)
    # how far apart the bounding spheres are (a plane: the sphere above it), negative: they overlap
    margin = float((pos2 - pos1) @ R1[:, 2] - B.rb) if A.type == hm.GEOM_PLANE else float(np.linalg.norm(pos2 - pos1) - (A.rb + B.rb))
    facts = dict(kind=f"{A.kind}-{B.kind}", plane=A.type == hm.GEOM_PLANE, ukind=ukind, okind=okind, g=g, gap=gap, dup=dup, depth=depth,
                 reach=1e-6 * float(A.aabb[3:].sum() + B.aabb[3:].sum()) + 2e-6, sphere_margin=margin)
    return w, facts


def control_of(w):
    """the negative control of a row: the same pair with every bh smaller by CTRL_BH and every radius by CTRL_RB"""
    c = w.copy()
    fl = c[10:56].view(np.float32).copy()
    fl[18:21] -= np.float32(CTRL_BH); fl[39:42] -= np.float32(CTRL_BH)
    fl[42] *= np.float32(1 - CTRL_RB); fl[43] *= np.float32(1 - CTRL_RB); fl[45] *= np.float32(1 - CTRL_RB)
    c[10:56] = fl.view(np.uint32)
    return c


def pack_rows(template):
    """rows that only exercise pair_pack: the radius bound of every candidate pair of every committed model, as the kernel forms it, and radii whose low 16 bits
    are 0x0000, 0x0001 and 0xffff"""
    rows, rads = [], []
    for name in MODELS:
        m = hm.load_config(name)
        rb = m.geom_rbound.astype(np.float32)
        for p in range(m.npair):
            g1, g2 = int(m.pair_geom1[p]), int(m.pair_geom2[p])
            rad = rb[g2] if int(m.geom_type[g1]) == hm.GEOM_PLANE else rb[g1] + rb[g2]
            rows.append((g1, g2, int(m.pair_fn[p]), np.float32(rad)))
    for base in (0.0117, 0.05, 0.3, 1.0, 1.7, 2.5, 3.999):
        hi = np.array([base], dtype=np.float32).view(np.uint32)[0] & np.uint32(0xFFFF0000)
        for k, low in enumerate((0x0000, 0x0001, 0xFFFF)):
            rows.append((63, 62 - k, k + 1, np.array([hi | np.uint32(low)], dtype=np.uint32).view(np.float32)[0]))
    out = []
    for g1, g2, fn, rad in rows:
        w = template.copy()
        w[6:9] = [g1, g2, fn]
        w[55] = np.array([rad], dtype=np.float32).view(np.uint32)[0]
        out.append(w); rads.append(rad)
    return out, [(r[0], r[1], r[2]) for r in rows], np.array(rads, dtype=np.float32)


def lane_off(i):
    return ((i // 64) & 1) == 1 and (i % 4) == 3


def layout(rows):
    """-> (words [n, 64] with n a multiple of 64, slot[k] = where row k went).  Lanes the harness switches off, and the tail, hold a filler (a copy of row 0)."""
    out, slot = [], []
    for w in rows:
        while lane_off(len(out)):
            out.append(rows[0])
        slot.append(len(out)); out.append(w)
    while len(out) % 64:
        out.append(rows[0])
    return np.stack(out).astype(np.uint32), np.array(slot)


@functools.lru_cache(maxsize=None)
def all_inputs():
    """dict(words, slot, facts (one dict per geometric row), n_geo, ctrl0 (first control row), pack0, pack_fields, pack_rads)"""
    rng = np.random.default_rng(950)
    S = shapes()
    rows, facts = [], []
    for a, b, reps in PAIRINGS:
        A, B = S[a], S[b]
        for _ in range(reps):
            for ukind in ((0,) if A.type == hm.GEOM_PLANE else (0, 1, 2)):
                for okind in range(5):
                    for g in GAPS:
                        w, f = make_row(rng, A, B, ukind, okind, g)
                        f["pair"] = f"{a}/{b}"
                        rows.append(w); facts.append(f)
    n_geo = len(rows)
    ctrl = [control_of(w) for w in rows]
    pk, fields, rads = pack_rows(rows[0])
    words, slot = layout(rows + ctrl + pk)
    return dict(words=words, slot=slot, facts=facts, n_geo=n_geo, ctrl0=n_geo, pack0=2 * n_geo, pack_fields=fields, pack_rads=rads)


# ------------------------------------------------------------------------------------------------ numpy fp32 restatement (self-test of this module only)
def emulate(words):
    """columns 0 .. 5 of the harness' output from a numpy fp32 restatement of sphere_hits_obb, obb_overlap, pair_cull and pair_cull_box_nb"""
    F = np.float32
    fl = np.ascontiguousarray(words[:, 10:56]).view(np.float32)
    t1 = words[:, 0]

    def geom(o):
        return fl[:, o:o + 3], fl[:, o + 3:o + 12].reshape(-1, 3, 3), fl[:, o + 15:o + 18], fl[:, o + 18:o + 21]
    p1, M1, c1, h1 = geom(0)
    p2, M2, c2, h2 = geom(21)
    rb1, rb2 = fl[:, 42], fl[:, 43]

    def sph(c, r, M, bc, bh):
        l = np.einsum("nji,nj->ni", M, c - bc)
        d = np.maximum(np.abs(l) - bh, F(0))
        return (d * d).sum(1, dtype=F) <= r * r

    def obb(M1, c1, h1, M2, c2, h2):
        d = c2 - c1
        ta = np.einsum("nji,nj->ni", M1, d)
        C = np.einsum("nki,nkj->nij", M1, M2)
        aC = np.abs(C) + F(1e-6)
        sep = np.zeros(len(d), bool)
        for i in range(3):
            sep |= np.abs(ta[:, i]) > h1[:, i] + (h2 * aC[:, i, :]).sum(1, dtype=F)
        for j in range(3):
            sep |= np.abs((ta * C[:, :, j]).sum(1, dtype=F)) > h2[:, j] + (h1 * aC[:, :, j]).sum(1, dtype=F)
        for i in range(3):
            for j in range(3):
                i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
                ra = h1[:, i1] * aC[:, i2, j] + h1[:, i2] * aC[:, i1, j]
                rb = h2[:, j1] * aC[:, i, j2] + h2[:, j2] * aC[:, i, j1]
                sep |= np.abs(ta[:, i2] * C[:, i1, j] - ta[:, i1] * C[:, i2, j]) > ra + rb
        return ~sep
    n = M1[:, :, 2]
    plane_val = ((c2 - p1) * n).sum(1, dtype=F) - (np.abs(np.einsum("nk,nkj->nj", n, M2)) * h2).sum(1, dtype=F)
    s12, s21, ov = sph(p2, rb2, M1, c1, h1), sph(p1, rb1, M2, c2, h2), obb(M1, c1, h1, M2, c2, h2)
    isp = t1 == hm.GEOM_PLANE
    r = p2 - p1
    cull = np.where(isp, (((r * n).sum(1, dtype=F)) <= rb2) & (plane_val <= 0), ((r * r).sum(1, dtype=F) <= (rb1 + rb2) ** 2) & s12 & s21 & ov)
    nb0 = np.where(isp, plane_val <= 0, s12 & s21 & ov)
    sk = F(SKIN)
    nbs = np.where(isp, plane_val <= sk, sph(p2, rb2 + sk, M1, c1, h1) & sph(p1, rb1 + sk, M2, c2, h2) & obb(M1, c1, h1 + sk, M2, c2, h2))
    return np.stack([s12, s21, ov, cull, nb0, nbs], 1).astype(np.uint32)


# ------------------------------------------------------------------------------------------------ judging the output words
SKIN0_COLS = {0: "sphere_hits_obb(2 in 1)", 1: "sphere_hits_obb(1 in 2)", 2: "obb_overlap", 3: "pair_cull", 4: "pair_cull_box_nb(0)"}
PLANE_COLS = (3, 4)                # what a plane-first pair is asked: the sphere / box functions read a plane's (empty) box and mean nothing there


def split(out, inp):
    """-> (geometric rows, their controls, pair_pack rows) of the harness' output [n, 16]"""
    out = np.asarray(out, dtype=np.uint32).reshape(-1, OUT_W)
    assert len(out) == len(inp["words"]), (len(out), len(inp["words"]))
    s, n = inp["slot"], inp["n_geo"]
    return out[s[:n]], out[s[n:2 * n]], out[s[2 * n:]]


def check_lanes(out, inp):
    """lanes behind the divergent branch keep the sentinel in every word; every other lane wrote every word"""
    out = np.asarray(out, dtype=np.uint32).reshape(-1, OUT_W)
    off = np.array([lane_off(i) for i in range(len(out))])
    assert off.sum() >= len(out) // 16, "no switched-off lanes in this run"
    assert np.all(out[off] == SENTINEL), f"rows {np.flatnonzero(np.any(out[off] != SENTINEL, 1))[:5]} of the switched-off lanes were written"
    assert not np.any(out[~off][:, :13] == SENTINEL), "a live lane left a word unwritten"
    assert np.all(out[~off][:, :6] <= 1)
    return int(off.sum())


def must_pass(facts):
    """per geometric row: (every skin = 0 function must pass, pair_cull_box_nb(HSR_SKIN) must pass)"""
    depth = np.array([f["depth"] for f in facts]); dup = np.array([f["dup"] for f in facts])
    plane = np.array([f["plane"] for f in facts]); gap = np.array([f["gap"] for f in facts])
    touch = np.nan_to_num(depth, nan=-1.0) >= DEMAND
    near = np.where(plane, gap <= SKIN - DEMAND, dup <= SKIN - DEMAND) | touch
    return touch, near


def false_rejects(rows, facts):
    """{column: indices of the rows that exact geometry says must pass and the function rejected}"""
    touch, near = must_pass(facts)
    plane = np.array([f["plane"] for f in facts])
    bad = {}
    for c in SKIN0_COLS:
        ask = touch & (~plane | (c in PLANE_COLS))
        bad[c] = np.flatnonzero(ask & (rows[:, c] == 0))
    bad[5] = np.flatnonzero(near & (rows[:, 5] == 0))
    return bad


def describe(facts, idx):
    return [{k: (round(v, 9) if isinstance(v, float) else v) for k, v in facts[i].items()} for i in idx[:4]]


def check_no_false_reject(rows, facts):
    touch, near = must_pass(facts)
    bad = false_rejects(rows, facts)
    for c, idx in bad.items():
        assert idx.size == 0, f"{SKIN0_COLS.get(c, 'pair_cull_box_nb(HSR_SKIN)')} rejected {idx.size} pairs that touch / are within the skin: {describe(facts, idx)}"
    return int(touch.sum()), int(near.sum())


def check_tightness(rows, facts):
    """box-box rows whose u is a face normal of the first box: the separation along a tested axis is exactly gap, so beyond the padding's reach the box culls must
    reject.  -> (rows asked at skin 0, at HSR_SKIN, {kind: smallest rejected gap at skin 0, smallest rejected gap at HSR_SKIN} over all rows)"""
    gap = np.array([f["gap"] for f in facts]); reach = np.array([f["reach"] for f in facts])
    face = np.array([f["kind"] == "box-box" and f["ukind"] == 1 for f in facts])
    ask0, asks = face & (gap > reach), face & (gap > SKIN + reach)
    for c in (2, 3, 4):
        idx = np.flatnonzero(ask0 & (rows[:, c] != 0))
        assert idx.size == 0, f"{SKIN0_COLS[c]} passed {idx.size} box pairs separated along a face normal by more than the padding reaches: {describe(facts, idx)}"
    idx = np.flatnonzero(asks & (rows[:, 5] != 0))
    assert idx.size == 0, f"pair_cull_box_nb(HSR_SKIN) passed {idx.size} box pairs farther apart along a face normal than skin + padding: {describe(facts, idx)}"
    frontier = {}
    for kind in sorted({f["kind"] for f in facts}):
        k = np.array([f["kind"] == kind for f in facts]) & (gap > 0)
        r0, rs = k & (rows[:, 4] == 0), k & (rows[:, 5] == 0)
        frontier[kind] = (float(gap[r0].min()) if r0.any() else None, float(gap[rs].min()) if rs.any() else None)
    return int(ask0.sum()), int(asks.sum()), frontier


def check_chain_and_persistent_agree(rows, facts):
    """pair_cull is pair_cull_box_nb(skin = 0) behind a bounding-sphere test (a plane: the sphere's distance).  Boxes: a sphere of radius |size| contains the
    box, so where the boxes pass the spheres pass, and the two verdicts are the same on every row.  Hulls and cylinders: the corners of the bounding box lie
    outside the bounding sphere, the sphere test can reject a pair whose boxes still overlap, and the persistent kernel makes that test in its level 1 - there
    pair_cull may only be the stricter of the two, and only where fp64 says the spheres are apart (or within 1e-6 of touching)."""
    n_same = n_sphere = 0
    for i, f in enumerate(facts):
        a, b = int(rows[i, 3]), int(rows[i, 4])
        if a == b:
            n_same += 1
            continue
        assert (a, b) == (0, 1), f"pair_cull passed a pair that pair_cull_box_nb(0) rejected: {describe(facts, [i])}"
        assert f["kind"] not in ("box-box", "plane-box"), f"pair_cull and pair_cull_box_nb(0) differ on boxes: {describe(facts, [i])}"
        assert f["sphere_margin"] > -1e-6, f"pair_cull rejected a pair whose bounding spheres overlap by {-f['sphere_margin']:.3e} and whose boxes pass: {describe(facts, [i])}"
        n_sphere += 1
    return n_same, n_sphere


def check_control(ctrl_rows, facts):
    """the same judgement on the rows with shrunken boxes and radii has to find false rejects in every function, or the judgement has no teeth"""
    bad = false_rejects(ctrl_rows, facts)
    counts = {c: int(idx.size) for c, idx in bad.items()}
    for c, k in counts.items():
        assert k > 0, f"toothless: boxes smaller by {CTRL_BH} and radii by {CTRL_RB:.0%} cost {SKIN0_COLS.get(c, 'pair_cull_box_nb(HSR_SKIN)')} not one touching pair"
    return counts


def check_pack(pack_rows_out, inp):
    """pair_pack keeps the upper 16 bits of the radius, rounded up: 7 mantissa bits survive, so rad <= R < rad (1 + 2^-7); geom and function fields round-trip;
    level 1 adds the skin to R in fp32"""
    rad = inp["pack_rads"].astype(np.float64)
    R = np.ascontiguousarray(pack_rows_out[:, 7]).view(np.float32)
    assert len(R) == len(rad)
    assert np.all(R.astype(np.float64) >= rad), f"packed radius below the radius: {rad[R < rad][:5]}"
    assert np.all(R.astype(np.float64) < rad * (1 + 2.0 ** -7)), f"packed radius a 2^-7 or more above: {rad[R >= rad * (1 + 2.0 ** -7)][:5]}"
    assert np.all((pack_rows_out[:, 6] & 0xFFFF0000) == pack_rows_out[:, 7])
    assert np.all(np.ascontiguousarray(pack_rows_out[:, 8]).view(np.float32) == R + np.float32(SKIN))
    assert np.all(np.ascontiguousarray(pack_rows_out[:, 12]).view(np.float32) == np.float32(SKIN)), "the harness was compiled with another HSR_SKIN than this module read"
    fields = np.array(inp["pack_fields"], dtype=np.uint32)
    assert np.array_equal(pack_rows_out[:, 9:12], fields), "geom / function fields do not round-trip"
    assert np.array_equal(pack_rows_out[:, 6] & 0x3FFF, fields[:, 0] | (fields[:, 1] << 6) | (fields[:, 2] << 12))
    exact = (inp["pack_rads"].view(np.uint32) & 0xFFFF) == 0
    assert np.all(R[exact] == inp["pack_rads"][exact]), "a radius that fits 16 bits was changed"
    return float(((R - rad) / rad).max()), int(exact.sum())
