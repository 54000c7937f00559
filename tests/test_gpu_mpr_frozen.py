"""support<8> and mpr_penetration<8> (csrc/collide.h) compile only the type arms a model's convex pairs can take (cv_types of cfg_consts.h), move
their scan winners with bound_ctrl DPP and compare the scan's slots past the end of a hull as copies of vertex 0.  tools/micro/mpr_frozen.hip runs them - with the masks every committed configuration has, and with any type
allowed as the generic kernel instances do - against a frozen copy of the previous form, one pair per 8-lane sub-group, and this module compares
hit, depth, dir, pos, sep, nsup, the three warm ids and the two plain support points of the margin rescan word by word.  Not one bit may differ.

Shapes, all from the committed cfg3 blob: the block box against the 27-vertex finger hulls (geoms 13, 15, 16), hull against hull (20, 27, 32, 40 and 45
vertices: one and two passes of the 32-wide scan), the wrist cylinder against the block box and against a hull, a hull against the box.  Poses (seeded):
the second shape is placed so that its support point against a direction u lies g along u from the first shape's - separated by exactly g for g > 0,
a vertex-to-vertex touch for g = 0 (the witness lies on a triangle edge: a warm-started run starts over), |g| <= 1e-6 on both sides, and overlaps from
1e-5 to 2 cm - or with its centre at a distance along u that sweeps from clear of the first shape to deep inside it (face contacts).  The binary runs
twice: the first pass starts every pair without a portal (zero ids); the second moves every pose a little and hands each pair the portal its first pass
ended on (valid ids), the portal of ANOTHER pose of the same two shapes (stale ids) or none.  The order of the rows decides which pairs share a wave:
shuffled, so that the eight sub-groups of a wave run different shapes, with a quarter of the pairs switched off behind a divergent branch in half of
the waves.  What the functions compute is pinned elsewhere (tests/test_narrowphase_geometry.py, tests/test_gpu_geometry.py); this module pins the BITS."""
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
IN_W, OUT_W = 48, 24
F32 = np.float32
BOX, CYL, MESH = 6, 5, 7
FIELDS = ["hit", "depth"] + [f"{n}.{c}" for n in ("dir", "pos", "sep") for c in "xyz"] + ["nsup", "warm0", "warm1", "warm2"] + [f"sup{k}.{c}" for k in (1, 2) for c in "xyz"] + ["pad"] * 3
# (first geom, second geom) of the cfg3 model: block box 17, finger hulls 13 / 15 / 16, palm and hand hulls 12 / 14 / 11 / 4, wrist cylinder 10
KINDS = [(17, 13), (17, 15), (17, 16), (13, 15), (12, 14), (11, 16), (4, 13), (14, 12), (10, 17), (10, 13), (16, 17)]
GAPS = [1e-2, 1e-3, 1e-5, 1e-6, 3e-7, 0.0, -3e-7, -1e-6, -1e-5, -1e-4, -1e-3, -5e-3, -2e-2]
CENTRE = [1.6, 1.2, 1.02, 1.0, 0.98, 0.9, 0.7, 0.4, 0.1]          # centre distance along u, in units of the sum of the two extents along u


def _rot(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


class Shapes:
    def __init__(self):
        sys.path.insert(0, str(ROOT))
        from hsr_env_amd.compiler import load_config
        a = load_config("cfg3").arrays
        self.type, self.nvert, self.adr = a["geom_type"], a["geom_meshnum"], a["geom_meshadr"]
        self.size = a["geom_size"].reshape(-1, 3)
        mv = a["mesh_vert"].reshape(-1, 3)
        self.verts = np.zeros((len(mv), 4), F32)
        self.verts[:, :3] = mv

    def points(self, g):
        """local points whose hull is the shape (the cylinder as 64 points per rim: only used to PLACE the shapes)"""
        t, s = self.type[g], self.size[g]
        if t == MESH: return self.verts[self.adr[g]:self.adr[g] + self.nvert[g], :3].astype(np.float64)
        if t == BOX: return np.array([[sx * s[0], sy * s[1], sz * s[2]] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
        ph = np.linspace(0, 2 * np.pi, 64, endpoint=False)
        return np.array([[s[0] * np.cos(p), s[0] * np.sin(p), z * s[1]] for p in ph for z in (-1, 1)])


def _row(sh, g1, g2, R1, p1, R2, p2, d, warm=(0, 0, 0), on=1):
    r = np.zeros(IN_W, np.uint32)
    f = r.view(F32)
    for k, g in enumerate((g1, g2)):
        mesh = sh.type[g] == MESH
        r[3 * k:3 * k + 3] = (sh.type[g], sh.nvert[g] if mesh else 0, sh.adr[g] if mesh else 0)
    r[6:9] = warm
    r[9] = on
    f[10:13] = p1; f[13:22] = R1.reshape(-1); f[22:25] = sh.size[g1]
    f[25:28] = p2; f[28:37] = R2.reshape(-1); f[37:40] = sh.size[g2]
    f[40:43] = d
    return r


def _poses(sh):
    """[(kind index, g1, g2, R1, p1, R2, p2, u)] - the first shape near the origin, the second placed against it along u"""
    rng = np.random.default_rng(20261)
    out = []
    for ki, (g1, g2) in enumerate(KINDS):
        P1, P2 = sh.points(g1), sh.points(g2)
        for rep in range(3):
            R1, R2 = _rot(rng), _rot(rng)
            p1 = rng.uniform(-0.3, 0.3, 3)
            u = rng.normal(size=3)
            u /= np.linalg.norm(u)
            W1, W2 = P1 @ R1.T + p1, P2 @ R2.T
            a = W1[np.argmax(W1 @ u)]
            b = W2[np.argmin(W2 @ u)]
            for g in GAPS:
                out.append((ki, g1, g2, R1, p1, R2, a + g * u - b, u))
            c1, c2 = W1.mean(0), W2.mean(0)
            ext = (W1 @ u).max() - c1 @ u + c2 @ u - (W2 @ u).min()
            for t in CENTRE:
                out.append((ki, g1, g2, R1, p1, R2, c1 + t * ext * u - c2, u))
    return out


def _run(exe, tmp_path, tag, rows, verts):
    fin, fvt, fout = tmp_path / f"{tag}_in.bin", tmp_path / "verts.bin", tmp_path / f"{tag}_out.bin"
    rows.tofile(fin)
    verts.tofile(fvt)
    r = subprocess.run([str(exe), str(fin), str(fvt), str(fout)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
    return np.fromfile(fout, np.uint32).reshape(3, len(rows), OUT_W)


def _compare(tag, rows, out):
    masked, generic, frozen = out
    on = rows[:, 9] != 0
    for name, new in (("masked", masked), ("generic", generic)):
        assert (new[~on] == 0xdeadbeef).all() and (frozen[~on] == 0xdeadbeef).all()
        bad = np.argwhere(new != frozen)
        for i, k in bad[:10]:
            print(f"{tag} {name}: row {i} (types {rows[i, 0]}/{rows[i, 3]}, nvert {rows[i, 1]}/{rows[i, 4]}, warm {rows[i, 6:9]}) {FIELDS[k]}: {new[i, k]:#010x} != frozen {frozen[i, k]:#010x}")
        print(f"{tag} {name}: {len(rows)} pairs, {int(on.sum())} switched on, mismatching words: {len(bad)}")
        assert len(bad) == 0


@pytest.mark.gpu
def test_support_and_mpr_bit_identical_to_the_frozen_form(tmp_path):
    sys.path.insert(0, str(ROOT))
    from hsr_env_amd.build import CODEGEN_FLAGS
    exe = tmp_path / "mpr_frozen"
    r = subprocess.run([HIPCC, *CODEGEN_FLAGS, "-w", "-o", str(exe), str(ROOT / "tools" / "micro" / "mpr_frozen.hip")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    sh = Shapes()
    poses = _poses(sh)
    rng = np.random.default_rng(20262)
    # ---- pass 1: no portal.  Shuffled; waves 0, 2, 4 .. have a quarter of their pairs switched off
    order = rng.permutation(len(poses))
    n1 = (len(order) + 7) // 8 * 8
    order = np.concatenate([order, order[:n1 - len(order)]])
    rows1 = np.stack([_row(sh, *poses[j][1:7], d=poses[j][7]) for j in order])
    off = (rng.uniform(size=n1) < 0.25) & ((np.arange(n1) // 8) % 2 == 0)
    rows1[off, 9] = 0
    out1 = _run(exe, tmp_path, "cold", rows1, sh.verts)
    _compare("cold", rows1, out1)
    fz = out1[2]
    on = rows1[:, 9] != 0
    hit = on & (fz[:, 0] == 1)
    depth = fz[:, 1].view(F32)
    sepn = np.abs(fz[:, 8:11].view(F32)).sum(1)
    kind = np.array([poses[j][0] for j in order])
    ids = fz[:, 12:15]
    vertex_pair = (rows1[:, 0] != CYL) & (rows1[:, 3] != CYL)
    print("cold pass: hits", int(hit.sum()), "depth < 1e-5", int((hit & (depth < 1e-5)).sum()), "1e-5 .. 1e-3", int((hit & (depth > 1e-5) & (depth < 1e-3)).sum()), "> 5e-3", int((hit & (depth > 5e-3)).sum()),
          "| separated with a direction", int((on & ~hit & (sepn > 0)).sum()), "| portals", int((hit & (ids[:, 0] > 0)).sum()), "| ended on an edge", int((hit & vertex_pair & (ids[:, 0] == 0)).sum()),
          "| supports per run: max", int(fz[on, 11].max()))
    # the poses reached what they were aimed at (read off the FROZEN functions' answers)
    assert (hit & (depth < 1e-5)).sum() >= 20 and (hit & (depth > 1e-5) & (depth < 1e-3)).sum() >= 20 and (hit & (depth > 5e-3)).sum() >= 20          # touching, shallow, deep
    assert (on & ~hit & (sepn > 0)).sum() >= 50                                                    # a separating direction proven
    for ki in range(len(KINDS)):
        assert (hit & (kind == ki)).any() and (on & ~hit & (kind == ki)).any(), KINDS[ki]
    assert (hit & (ids[:, 0] > 0)).sum() >= 50 and not (ids[~vertex_pair & on] != 0).any()          # portals to hand on; a cylinder has no vertex ids
    assert (hit & vertex_pair & (ids[:, 0] == 0)).sum() >= 10                                        # runs that ended on a triangle edge
    # ---- pass 2: every pose moved a little; its own portal, the portal of another pose of the same shapes, or none
    have = {j: ids[k].copy() for k, j in enumerate(order) if on[k] and hit[k] and ids[k, 0] > 0}
    by_kind = {}
    for j in have: by_kind.setdefault(poses[j][0], []).append(j)
    rows2, mode = [], []
    for j, (ki, g1, g2, R1, p1, R2, p2, u) in enumerate(poses):
        for variant in range(2):
            dp = rng.normal(size=3) * (1e-5 if variant == 0 else 3e-4)
            d = u + rng.normal(size=3) * 0.05
            if j in have:
                rows2.append(_row(sh, g1, g2, R1, p1, R2, p2 + dp, d, warm=have[j])); mode.append("valid")
            if ki in by_kind and len(by_kind[ki]) > 1:
                other = by_kind[ki][int(rng.integers(len(by_kind[ki])))]
                if other != j: rows2.append(_row(sh, g1, g2, R1, p1, R2, p2 + dp, d, warm=have[other])); mode.append("stale")
            if variant == 0: rows2.append(_row(sh, g1, g2, R1, p1, R2, p2 + dp, d)); mode.append("zero")
    perm = rng.permutation(len(rows2))
    n2 = len(perm) // 8 * 8
    rows2 = np.stack([rows2[k] for k in perm[:n2]])
    mode = np.array([mode[k] for k in perm[:n2]])
    off = (rng.uniform(size=n2) < 0.25) & ((np.arange(n2) // 8) % 2 == 0)
    rows2[off, 9] = 0
    out2 = _run(exe, tmp_path, "warm", rows2, sh.verts)
    _compare("warm", rows2, out2)
    fz = out2[2]
    on = rows2[:, 9] != 0
    hit = on & (fz[:, 0] == 1)
    nsup = fz[:, 11].astype(np.int64)
    valid = on & (mode == "valid")
    print("warm pass: valid", int(valid.sum()), "stale", int((on & (mode == "stale")).sum()), "zero", int((on & (mode == "zero")).sum()),
          "| valid runs with at most 2 supports", int((valid & hit & (nsup <= 2)).sum()), "| valid runs that ended on an edge", int((valid & hit & (fz[:, 12] == 0)).sum()))
    assert valid.sum() >= 100 and (on & (mode == "stale")).sum() >= 100 and (on & (mode == "zero")).sum() >= 100
    assert (valid & hit & (nsup <= 2)).sum() >= 20          # the warm start confirmed the old face
    assert (valid & hit & (fz[:, 12] == 0)).sum() >= 5      # a warm run whose witness was not interior: it started over
    assert len(rows1) + len(rows2) >= 2000
