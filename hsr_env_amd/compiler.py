"""Offline model compiler: HSR MJCF (+ STL meshes) -> flat constant tables ("model blob").

This is the build's counterpart of ``mujoco_py.load_model_from_path`` applied to the XML that
``hsr.util.mutate_xml`` would have produced (reference: hsr/mujoco_env.py:33-34,
hsr/util.py:87-182).  It runs once, on the host, in fp64, and needs the reference's *data*
files (hsr/models/world.xml, hsr/models/hsr.mjcf, hsr/hsr_meshes/meshes/**/*.stl); the GPU box
only ever sees the compiled blobs committed under ``hsr_env_amd/models/``.

What it does (decisions H1-H7 of SURVEY.md §7 are recorded in ``Model.meta``):
  * applies the reference's XML mutations directly: block injection (util.py:106-127) and the
    ``--use-dof`` actuator/joint filter (util.py:137-146);
  * resolves defaults (second top-level ``<default class="all">`` applies to all geoms, H3),
    ``angle="degree"`` (H4), ``inertiafromgeom="true"`` (H2), malformed ``pos`` (H1),
    unnormalised quaternions (H5);
  * folds every joint-less body into its nearest jointed ancestor ("link" = MuJoCo weld body),
    so the device tables hold <= 1 + 5 + n_blocks rigid links instead of ~50 bodies;
  * computes convex hulls of collidable meshes, geom bounding spheres, the static candidate
    geom-pair list after MuJoCo's filters (same weld body, parent-child weld bodies unless the
    parent is the world, <exclude>, contype/conaffinity);
  * computes qpos0 statistics used by the constraint regulariser (body/dof invweight0,
    meaninertia).

Engine semantics are restated from MuJoCo's public documentation (the engine itself is absent
from the reference tree and from this container) - parity with mujoco-py is
therefore unpinned; see DESIGN.md.

``compile_model`` is the list of stages.  The blob container ``Model``, the table layout and the
numpy reference the last stage uses are model.py's (what the run time imports); its names stay
importable from here.
"""
from __future__ import annotations

import re
import struct
import xml.etree.ElementTree as ET
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np

from .model import (BLOB_MAGIC, DOF_FREE_ANG, DOF_FREE_LIN, DOF_HINGE, DOF_SLIDE,  # noqa: F401
                    FN_BOX_BOX, FN_CONVEX, FN_MAXCON, FN_PLANE_BOX, FN_PLANE_CONVEX,
                    GEOM_BOX, GEOM_CYLINDER, GEOM_MESH, GEOM_PLANE, GEOM_SPHERE, MODEL_DIR, UNLIMITED, _ARRAY_FIELDS,
                    OPT_GRAV_Z, OPT_IMPRATIO, OPT_ITERATIONS, OPT_LS_ITERATIONS, OPT_LS_TOLERANCE, OPT_MEANINERTIA,
                    OPT_MPR_ITERATIONS, OPT_MPR_TOLERANCE, OPT_TIMESTEP, OPT_TOLERANCE,
                    SZ_NBODY, SZ_NCONMAX, SZ_NDENSE, SZ_NGEOM, SZ_NJMAX, SZ_NLIMIT, SZ_NLINK, SZ_NMESHVERT, SZ_NMOCAP,
                    SZ_NPAIR, SZ_NQ, SZ_NSLOT, SZ_NU, SZ_NV,
                    Model, axis_angle_quat, dof_motion, link_kinematics, load_config, mass_matrix, point_jacobian,
                    quat_mul, quat_normalize, quat_to_mat)

GEOM_TYPES = {"plane": GEOM_PLANE, "sphere": GEOM_SPHERE, "cylinder": GEOM_CYLINDER,
              "box": GEOM_BOX, "mesh": GEOM_MESH}

DEFAULT_REF_ROOT = Path("/root/reference/hsr")
ALL_DOFS = ["slide_x", "slide_y", "arm_lift_joint", "arm_flex_joint", "wrist_roll_joint",
            "hand_l_proximal_joint", "hand_r_proximal_joint"]


def _vec(text, n, default):
    """Parse an MJCF float vector; malformed text (H1: pos="0 0hsr") falls back to default."""
    if text is None:
        return np.array(default, dtype=np.float64)
    try:
        v = np.array([float(t) for t in text.split()], dtype=np.float64)
    except ValueError:
        return np.array(default, dtype=np.float64)
    if v.size != n:
        if v.size < n and n == 3 and v.size >= 1:   # geom size with fewer entries
            out = np.zeros(n)
            out[:v.size] = v
            return out
        return np.array(default, dtype=np.float64)
    return v


# ----------------------------------------------------------------------------- mesh handling
def load_stl(path: Path) -> np.ndarray:
    """Binary STL -> triangles [n,3,3] (fp64)."""
    raw = path.read_bytes()
    n = struct.unpack("<I", raw[80:84])[0]
    rec = np.dtype([("n", "<3f4"), ("v", "<9f4"), ("a", "<u2")])
    arr = np.frombuffer(raw, dtype=rec, count=n, offset=84)
    return arr["v"].reshape(n, 3, 3).astype(np.float64)


def mesh_inertia_legacy(tris: np.ndarray):
    """MuJoCo's legacy mesh inertia: pyramids from the surface centroid to every face, |volume|.

    Returns (volume, com[3], inertia about com [3,3]) for unit density.
    """
    a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    center = ((a + b + c) / 3.0 * area[:, None]).sum(0) / area.sum()
    a0, b0, c0 = a - center, b - center, c - center
    vol = np.abs(np.einsum("ij,ij->i", a0, np.cross(b0, c0))) / 6.0
    V = vol.sum()
    # tetra (0,a0,b0,c0): centroid (a0+b0+c0)/4 ; second moment about the apex:
    # int x x^T dV = vol/20 * (sum_i v_i v_i^T + (sum v)(sum v)^T)
    cen = (a0 + b0 + c0) / 4.0
    com0 = (cen * vol[:, None]).sum(0) / V
    s = a0 + b0 + c0
    P = (np.einsum("n,ni,nj->ij", vol, a0, a0) + np.einsum("n,ni,nj->ij", vol, b0, b0) +
         np.einsum("n,ni,nj->ij", vol, c0, c0) + np.einsum("n,ni,nj->ij", vol, s, s)) / 20.0
    # covariance about the pyramid apex (center) -> about com
    P -= V * np.outer(com0, com0)
    inertia = np.trace(P) * np.eye(3) - P
    return V, center + com0, inertia


def convex_hull_vertices(points: np.ndarray) -> np.ndarray:
    from scipy.spatial import ConvexHull
    uniq = np.unique(points.round(9), axis=0)
    hull = ConvexHull(uniq)
    return uniq[np.sort(hull.vertices)]


# ----------------------------------------------------------------------------- MJCF records
@dataclass
class _Geom:
    name: str
    type: int
    size: np.ndarray
    pos: np.ndarray
    quat: np.ndarray
    mesh: Optional[str]
    contype: int
    conaffinity: int
    condim: int
    friction: np.ndarray
    solref: np.ndarray
    solimp: np.ndarray
    mass: Optional[float]
    density: float


@dataclass
class _Joint:
    name: str
    type: str            # slide | hinge | free
    axis: np.ndarray
    pos: np.ndarray
    limited: bool
    range: np.ndarray
    damping: float


@dataclass
class _Body:
    name: str
    pos: np.ndarray
    quat: np.ndarray
    mocap: bool
    parent: int
    joints: List[_Joint] = field(default_factory=list)
    geoms: List[_Geom] = field(default_factory=list)
    inertial: Optional[dict] = None


@dataclass
class _Parsed:
    """What the model needs of the mutated MJCF tree."""
    opt: dict
    bodies: List[_Body]
    meshes: Dict[str, Path]
    excludes: list
    inertiafromgeom: bool
    meta: dict


# ----------------------------------------------------------------------------- the reference's XML mutations
def _block_positions(block_pos, n_blocks: int) -> np.ndarray:
    if block_pos is None:
        # resting height on the pan: 0.405 + 0.017 (world.xml:83-84, util.py:120)
        block_pos = [[0.0, 0.12 * (i - (n_blocks - 1) / 2.0), 0.422] for i in range(n_blocks)]
    return np.asarray(block_pos, dtype=np.float64).reshape(n_blocks, 3)


def _inject_blocks(worldbody, block_pos, block_geom=None):
    """hsr/util.py:106-127: one free body `block<i>` with one geom per row of block_pos."""
    for i, pos in enumerate(block_pos):
        name = f"block{i}"
        body = ET.SubElement(worldbody, "body", attrib=dict(name=name, pos=" ".join(repr(float(x)) for x in pos)))
        gattr = dict(name=name, type="box", mass="1", size=".05 .025 .017", condim="6", solimp="0.99 0.99 0.01", solref="0.01 1")
        if block_geom:              # test scenes only: another shape for the injected body (e.g. one of the robot's hulls as a free body)
            gattr.update(block_geom)
            if gattr.get("type") == "mesh":
                gattr.pop("size", None)
        ET.SubElement(body, "geom", attrib=gattr)
        ET.SubElement(body, "freejoint", attrib=dict(name=f"block{i}joint"))


def _apply_setters(root, set_xml):
    """hsr/util.py:129-135 (`for change in changes`): the path's last component is the attribute, the rest an ElementTree
    path relative to the root of the file being mutated; a path that matches nothing in this file is skipped."""
    for path, value in set_xml:
        parent = re.sub('/[^/]*$', '', str(path))
        elt = root.find(parent)
        if isinstance(elt, ET.Element):
            elt.set(re.search('[^/]*$', str(path))[0], str(value))


def _filter_dofs(root, dofs) -> list:
    """hsr/util.py:137-146 (`--use-dof`): removes the actuators and joints of every other dof -> the actuators that stay."""
    kept = []
    for acts in root.iter("actuator"):
        for a in list(acts):
            if a.get("joint") in dofs:
                kept.append(a)
            else:
                acts.remove(a)
    for body in root.iter("body"):
        for j in body.findall("joint"):
            if j.get("name") not in dofs:
                body.remove(j)
    return kept


def _mutated_tree(xml_path: Path, dofs, block_pos, set_xml, block_geom):
    """The tree mujoco-py would have loaded -> (root, actuator elements): block injection, then the --set-xml changes, file by
    file as mutate_tree does, with the included files spliced in (util.py:148-151 keeps includes relative), then the dof filter."""
    root = ET.parse(xml_path).getroot()
    worldbody = root.find("worldbody")
    _inject_blocks(worldbody, block_pos, block_geom)
    _apply_setters(root, set_xml)
    for i, child in enumerate(list(worldbody)):
        if child.tag == "include":
            inc = ET.parse(xml_path.parent / child.get("file")).getroot()
            _apply_setters(inc, set_xml)
            worldbody.remove(child)
            for j, b in enumerate(list(inc)):
                worldbody.insert(i + j, b)
    return root, _filter_dofs(root, dofs)


# ----------------------------------------------------------------------------- reading the tree
def _read_options(root) -> dict:
    opt = {"timestep": 0.002, "impratio": 1.0, "cone": "pyramidal"}
    for o in root.findall("option"):
        for k in ("timestep", "impratio"):
            if o.get(k) is not None:
                opt[k] = float(o.get(k))
        if o.get("cone") is not None:
            opt["cone"] = o.get("cone")
    size = root.find("size")
    opt["njmax"] = int(size.get("njmax", 500))
    opt["nconmax"] = int(size.get("nconmax", 100))
    return opt


@dataclass
class _BodyReader:
    """Walks the body tree depth first into `bodies`; geom attributes resolve global default < class default < own (H3)."""
    degree: bool
    geom_global: Dict[str, str]
    geom_class: Dict[str, Dict[str, str]]
    bodies: List[_Body]
    meta: dict
    ngeom: int = 0

    def geom(self, g) -> _Geom:
        at = dict(self.geom_global)
        at.update(self.geom_class.get(g.get("class"), {}))
        at.update(g.attrib)
        solimp = np.array([0.9, 0.95, 0.001, 0.5, 2.0])
        if "solimp" in at:
            v = [float(t) for t in at["solimp"].split()]
            solimp[:len(v)] = v
        fr = np.array([1.0, 0.005, 0.0001])
        if "friction" in at:
            v = [float(t) for t in at["friction"].split()]
            fr[:len(v)] = v
        self.ngeom += 1
        return _Geom(name=at.get("name", f"geom{self.ngeom - 1}"), type=GEOM_TYPES[at.get("type", "sphere")],
                     size=_vec(at.get("size"), 3, [0, 0, 0]),
                     pos=_vec(at.get("pos"), 3, [0, 0, 0]),
                     quat=quat_normalize(_vec(at.get("quat"), 4, [1, 0, 0, 0])),
                     mesh=at.get("mesh"), contype=int(at.get("contype", 1)),
                     conaffinity=int(at.get("conaffinity", 1)), condim=int(at.get("condim", 3)),
                     friction=fr, solref=_vec(at.get("solref"), 2, [0.02, 1.0]), solimp=solimp,
                     mass=float(at["mass"]) if "mass" in at else None,
                     density=float(at.get("density", 1000.0)))

    def joint(self, j) -> _Joint:
        if j.tag == "freejoint":
            return _Joint(name=j.get("name"), type="free", axis=np.zeros(3), pos=np.zeros(3), limited=False,
                          range=np.zeros(2), damping=0.0)
        jt = j.get("type", "hinge")
        rng = _vec(j.get("range"), 2, [0, 0])
        if jt == "hinge" and self.degree:
            rng = np.deg2rad(rng)
        return _Joint(name=j.get("name"), type=jt,
                      axis=quat_normalize(_vec(j.get("axis"), 3, [0, 0, 1])),
                      pos=_vec(j.get("pos"), 3, [0, 0, 0]),
                      limited=j.get("limited", "false") == "true", range=rng,
                      damping=float(j.get("damping", 0.0)))

    def body(self, b, parent_id: int) -> _Body:
        body = _Body(name=b.get("name"), pos=_vec(b.get("pos"), 3, [0, 0, 0]),
                     quat=quat_normalize(_vec(b.get("quat"), 4, [1, 0, 0, 0])),
                     mocap=b.get("mocap", "false") == "true", parent=parent_id)
        if b.get("pos") is not None and _vec(b.get("pos"), 3, [np.nan] * 3)[0] != body.pos[0]:
            self.meta.setdefault("H1_malformed_pos", []).append(b.get("name"))
        body.joints = [self.joint(j) for j in b.findall("joint")] + [self.joint(j) for j in b.findall("freejoint")]
        inert = b.find("inertial")
        if inert is not None:
            body.inertial = dict(pos=_vec(inert.get("pos"), 3, [0, 0, 0]),
                                 quat=quat_normalize(_vec(inert.get("quat"), 4, [1, 0, 0, 0])),
                                 mass=float(inert.get("mass")),
                                 diag=_vec(inert.get("diaginertia"), 3, [0, 0, 0]))
        return body

    def walk(self, elem, parent_id: int):
        self.bodies[parent_id].geoms += [self.geom(g) for g in elem.findall("geom")]
        for b in elem.findall("body"):
            self.bodies.append(self.body(b, parent_id))
            self.walk(b, len(self.bodies) - 1)


def _read_tree(root, xml_path: Path) -> _Parsed:
    comp = root.find("compiler")
    meshdir = (xml_path.parent / comp.get("meshdir", ".")).resolve()
    reader = _BodyReader(degree=comp.get("angle", "degree") == "degree", geom_global={}, geom_class={}, meta={},
                         bodies=[_Body("world", np.zeros(3), np.array([1., 0, 0, 0]), False, -1)])
    for top in root.findall("default"):
        for g in top.findall("geom"):
            reader.geom_global.update(g.attrib)
        for sub in top.findall("default"):
            for g in sub.findall("geom"):
                reader.geom_class.setdefault(sub.get("class"), {}).update(g.attrib)
    reader.walk(root.find("worldbody"), 0)
    return _Parsed(opt=_read_options(root), bodies=reader.bodies, meta=reader.meta,
                   meshes={m.get("name"): meshdir / m.get("file") for m in root.find("asset").findall("mesh")},
                   excludes=[(e.get("body1"), e.get("body2")) for c in root.findall("contact") for e in c.findall("exclude")],
                   inertiafromgeom=comp.get("inertiafromgeom", "auto") == "true")


# ----------------------------------------------------------------------------- compile: records of the stages
@dataclass
class _Mesh:
    volume: float
    com: np.ndarray
    inertia: np.ndarray      # about com, unit density
    hull: np.ndarray


class _MeshCache:
    """Mass properties (MuJoCo's legacy rule) and convex hull per mesh name; every STL file is read once."""

    def __init__(self, files: Dict[str, Path]):
        self.files, self.data = files, {}

    def __getitem__(self, name: str) -> _Mesh:
        if name not in self.data:
            tris = load_stl(self.files[name])
            self.data[name] = _Mesh(*mesh_inertia_legacy(tris), convex_hull_vertices(tris.reshape(-1, 3)))
        return self.data[name]


@dataclass
class _Shape:
    """A geom's shape in its own frame, unit density."""
    volume: float
    inertia: np.ndarray      # about the centre
    rbound: float
    size: np.ndarray
    aabb: np.ndarray         # box containing the geom: centre(3) + half extents(3); tight (asymmetric) for hulls
    com: np.ndarray = field(default_factory=lambda: np.zeros(3))     # the centre: the frame origin except for a mesh
    verts: Optional[np.ndarray] = None                               # mesh: hull vertices about the centre


@dataclass
class _MassProps:
    mass: float = 0.0
    com: np.ndarray = field(default_factory=lambda: np.zeros(3))
    inertia: np.ndarray = field(default_factory=lambda: np.zeros((3, 3)))      # about com


@dataclass
class _Link:
    body: int                # the jointed body that heads the link
    parent: int
    pos: np.ndarray          # in the parent link's frame
    quat: np.ndarray
    inertial: _MassProps = field(default_factory=_MassProps)         # in the link frame
    dofadr: int = 0          # the next four: written by assign_dofs
    dofnum: int = 0
    qposadr: int = 0
    free: int = 0


@dataclass
class _Fold:
    links: List[_Link]
    body_link: np.ndarray
    body_pos: np.ndarray     # pose of every joint-less body in its link's frame (identity for the body that heads a link)
    body_quat: np.ndarray


@dataclass
class _Dof:
    link: int
    type: int
    axis: np.ndarray
    pos: np.ndarray
    parent: int
    damping: float
    qposadr: int
    limited: int
    range: np.ndarray


@dataclass
class _JointAddr:
    name: str
    qposadr: int
    nq: int                  # 7: free joint, 1: slide / hinge
    dofadr: int


@dataclass
class _CollGeom:
    name: str
    geom: _Geom              # contype / conaffinity / condim / friction / solref / solimp as parsed
    link: int
    body: int
    pos: np.ndarray          # in the link frame
    quat: np.ndarray
    shape: _Shape
    meshadr: int
    meshnum: int


@dataclass
class _Pair:
    g1: int
    g2: int
    fn: int
    condim: int
    friction: np.ndarray
    solref: np.ndarray
    solimp: np.ndarray


# ----------------------------------------------------------------------------- compile: the stages
def geom_shape(g: _Geom, meshes: _MeshCache) -> _Shape:
    """The one place that knows the geom types."""
    s = g.size
    if g.type == GEOM_PLANE:
        return _Shape(0.0, np.zeros((3, 3)), 0.0, s, np.zeros(6))
    if g.type == GEOM_BOX:
        a, b, c = s
        vol = 8 * a * b * c
        return _Shape(vol, vol / 3.0 * np.diag([b * b + c * c, a * a + c * c, a * a + b * b]), np.linalg.norm(s), s,
                      np.concatenate([np.zeros(3), s]))
    if g.type == GEOM_SPHERE:
        r = s[0]
        vol = 4.0 / 3.0 * np.pi * r ** 3
        return _Shape(vol, 0.4 * vol * r * r * np.eye(3), r, s, np.array([0, 0, 0, r, r, r]))
    if g.type == GEOM_CYLINDER:
        r, hh = s[0], s[1]
        vol = np.pi * r * r * 2 * hh
        ixx = vol * (3 * r * r + 4 * hh * hh) / 12.0
        return _Shape(vol, np.diag([ixx, ixx, 0.5 * vol * r * r]), np.hypot(r, hh), s, np.array([0, 0, 0, r, r, hh]))
    if g.type == GEOM_MESH:
        md = meshes[g.mesh]
        verts = md.hull - md.com
        lo, hi = verts.min(0), verts.max(0)
        return _Shape(md.volume, md.inertia, np.linalg.norm(verts, axis=1).max(), np.abs(verts).max(0),
                      np.concatenate([(lo + hi) / 2, (hi - lo) / 2]), com=md.com, verts=verts)
    raise ValueError(g.type)


def _geom_mass_props(g: _Geom, meshes: _MeshCache):
    """-> (mass, com in body frame, inertia about com in body frame)"""
    sh = geom_shape(g, meshes)
    if g.type == GEOM_PLANE:
        return 0.0, np.zeros(3), np.zeros((3, 3))
    Rg = quat_to_mat(g.quat)
    mass = g.mass if g.mass is not None else g.density * sh.volume
    scale = mass / sh.volume
    return mass, g.pos + Rg @ sh.com, Rg @ (sh.inertia * scale) @ Rg.T


def _combine(parts) -> _MassProps:
    """Rigidly joined (mass, com, inertia about com) parts in one frame; the sums run in the order given."""
    mtot = sum(p[0] for p in parts)
    com = sum(p[0] * p[1] for p in parts) / mtot
    I = np.zeros((3, 3))
    for mm, c, Ic in parts:
        d = c - com
        I += Ic + mm * (d @ d * np.eye(3) - np.outer(d, d))
    return _MassProps(mtot, com, I)


def body_inertias(bodies: List[_Body], inertiafromgeom: bool, meshes: _MeshCache) -> List[_MassProps]:
    """Mass properties of every body in its own frame: from its geoms (H2), else from its <inertial>."""
    out = [_MassProps()]
    for b in bodies[1:]:
        parts = [_geom_mass_props(g, meshes) for g in b.geoms] if inertiafromgeom else []
        parts = [p for p in parts if p[0] > 0]
        if parts:
            out.append(_combine(parts))
        elif b.inertial is not None:
            Ri = quat_to_mat(b.inertial["quat"])
            out.append(_MassProps(b.inertial["mass"], b.inertial["pos"], Ri @ np.diag(b.inertial["diag"]) @ Ri.T))
        else:
            out.append(_MassProps())
    return out


def fold_links(bodies: List[_Body], inertials: List[_MassProps]) -> _Fold:
    """Every joint-less body becomes part of its nearest jointed ancestor's link (link 0: the world)."""
    nb = len(bodies)
    body_link = np.zeros(nb, dtype=np.int32)
    body_pos = np.zeros((nb, 3)); body_quat = np.tile([1., 0, 0, 0], (nb, 1))
    links = [_Link(body=0, parent=0, pos=np.zeros(3), quat=np.array([1., 0, 0, 0]))]
    for i in range(1, nb):
        b = bodies[i]
        p = b.parent
        # pose of this body in its parent's link frame
        Rp = quat_to_mat(body_quat[p])
        pos_in_l = body_pos[p] + Rp @ b.pos
        quat_in_l = quat_normalize(quat_mul(body_quat[p], b.quat))
        if b.joints:
            links.append(_Link(body=i, parent=int(body_link[p]), pos=pos_in_l, quat=quat_in_l))
            body_link[i] = len(links) - 1
        else:
            body_link[i] = body_link[p]
            body_pos[i], body_quat[i] = pos_in_l, quat_in_l
    for l in range(1, len(links)):
        parts = []
        for i in range(nb):
            if body_link[i] == l and inertials[i].mass > 0:
                Rb = quat_to_mat(body_quat[i])
                parts.append((inertials[i].mass, body_pos[i] + Rb @ inertials[i].com, Rb @ inertials[i].inertia @ Rb.T))
        links[l].inertial = _combine(parts)
    return _Fold(links, body_link, body_pos, body_quat)


def assign_dofs(bodies: List[_Body], links: List[_Link]):
    """-> (dofs, qpos0, joint addresses), joints in link order; writes each link's dofadr / dofnum / qposadr / free."""
    dofs: List[_Dof] = []
    qpos0: list = []
    joints: List[_JointAddr] = []
    last_dof_of_link = {0: -1}
    for l, lk in enumerate(links):
        if l == 0:
            continue
        b = bodies[lk.body]
        lk.dofadr, lk.qposadr = len(dofs), len(qpos0)
        prev = last_dof_of_link[lk.parent]
        for j in b.joints:
            if j.type == "free":
                assert len(b.joints) == 1 and lk.parent == 0
                lk.free = 1
                joints.append(_JointAddr(j.name, len(qpos0), 7, len(dofs)))
                qa = len(qpos0)
                qpos0 += list(lk.pos) + list(lk.quat)
                for k in range(6):
                    # translational dofs address qpos[qa+k]; rotational ones the quaternion start
                    dofs.append(_Dof(link=l, type=DOF_FREE_LIN if k < 3 else DOF_FREE_ANG, axis=np.eye(3)[k % 3], pos=np.zeros(3),
                                     parent=prev, damping=0.0, qposadr=qa + k if k < 3 else qa + 3, limited=0, range=np.zeros(2)))
                    prev = len(dofs) - 1
            else:
                joints.append(_JointAddr(j.name, len(qpos0), 1, len(dofs)))
                dofs.append(_Dof(link=l, type=DOF_SLIDE if j.type == "slide" else DOF_HINGE, axis=j.axis, pos=j.pos, parent=prev,
                                 damping=j.damping, qposadr=len(qpos0), limited=int(j.limited), range=j.range))
                prev = len(dofs) - 1
                qpos0.append(0.0)
        lk.dofnum = len(dofs) - lk.dofadr
        last_dof_of_link[l] = prev
        # a non-free link may hold several slides or exactly one hinge (keeps dof axes = final frame)
        types = [d.type for d in dofs[lk.dofadr:]]
        assert lk.free or types.count(DOF_HINGE) == 0 or len(types) == 1, "mixed joints on a body"
    return dofs, qpos0, joints


def collidable_geoms(bodies: List[_Body], fold: _Fold, meshes: _MeshCache):
    """-> (geoms with a contype or conaffinity bit, placed in their link's frame; hull vertices of the mesh geoms, concatenated)"""
    geoms: List[_CollGeom] = []
    mesh_vert = []
    for i, b in enumerate(bodies):
        for g in b.geoms:
            if g.contype == 0 and g.conaffinity == 0:
                continue
            Rb = quat_to_mat(fold.body_quat[i])
            pos = fold.body_pos[i] + Rb @ g.pos
            quat = quat_normalize(quat_mul(fold.body_quat[i], g.quat))
            sh = geom_shape(g, meshes)
            meshadr, meshnum = 0, 0
            if sh.verts is not None:
                # geom frame origin := mesh centre of mass (MuJoCo recentres meshes)
                pos = pos + quat_to_mat(quat) @ sh.com
                meshadr, meshnum = sum(len(v) for v in mesh_vert), len(sh.verts)
                mesh_vert.append(sh.verts)
            geoms.append(_CollGeom(name=g.name if g.mesh is None else f"{b.name}:{g.mesh}", geom=g, link=int(fold.body_link[i]),
                                   body=i, pos=pos, quat=quat, shape=sh, meshadr=meshadr, meshnum=meshnum))
    return geoms, (np.concatenate(mesh_vert) if mesh_vert else np.zeros((0, 3)))


def _may_collide(ga: _CollGeom, gc: _CollGeom, links: List[_Link], bodies: List[_Body], excl) -> bool:
    """MuJoCo's filters: same weld body, parent-child weld bodies unless the parent is the world, <exclude>, contype/conaffinity."""
    la, lc = ga.link, gc.link
    if la == lc:
        return False
    if (links[la].parent == lc and lc != 0) or (links[lc].parent == la and la != 0):
        return False
    if frozenset((bodies[ga.body].name, bodies[gc.body].name)) in excl:
        return False
    return bool((ga.geom.contype & gc.geom.conaffinity) or (gc.geom.contype & ga.geom.conaffinity))


def candidate_pairs(geoms: List[_CollGeom], links: List[_Link], bodies: List[_Body], excludes) -> List[_Pair]:
    """The static candidate list, the geom of the lower type first, with the pair's mixed contact parameters."""
    excl = {frozenset(e) for e in excludes}
    pairs = []
    for a in range(len(geoms)):
        for c in range(a + 1, len(geoms)):
            if not _may_collide(geoms[a], geoms[c], links, bodies, excl):
                continue
            g1, g2 = (a, c) if geoms[a].geom.type <= geoms[c].geom.type else (c, a)
            A, B = geoms[g1].geom, geoms[g2].geom
            if A.type == GEOM_PLANE:
                fn = FN_PLANE_BOX if B.type == GEOM_BOX else FN_PLANE_CONVEX
            elif A.type == GEOM_BOX and B.type == GEOM_BOX:
                fn = FN_BOX_BOX
            else:
                fn = FN_CONVEX
            fr = np.maximum(A.friction, B.friction)
            pairs.append(_Pair(g1=g1, g2=g2, fn=fn, condim=max(A.condim, B.condim),
                               friction=np.array([fr[0], fr[0], fr[1], fr[2], fr[2]]),
                               solref=0.5 * (A.solref + B.solref), solimp=0.5 * (A.solimp + B.solimp)))
    return pairs


def pair_slots(pairs: List[_Pair], plane_convex_points: int) -> np.ndarray:
    """First contact slot of every pair (and, last, their number)."""
    slot = np.zeros(len(pairs) + 1, dtype=np.int32)
    for i, p in enumerate(pairs):
        slot[i + 1] = slot[i] + (plane_convex_points if p.fn == FN_PLANE_CONVEX else FN_MAXCON[p.fn])
    return slot


def _act_range(a, key, flag):
    if a.get(flag, "false") != "true" or a.get(key) is None:
        return [-UNLIMITED, UNLIMITED]
    return _vec(a.get(key), 2, [0, 0])


def actuator_tables(acts, joints: List[_JointAddr]) -> Dict[str, np.ndarray]:
    joint_names = [j.name for j in joints]
    # MuJoCo clamps ctrl / actuator force only when ctrllimited / forcelimited is set (world.xml:104-124 sets both on all seven
    # actuators); an unlimited actuator gets an effectively infinite range so that the kernels' unconditional clamp is a no-op
    return dict(
        act_dof=np.array([joints[joint_names.index(a.get("joint"))].dofadr for a in acts], dtype=np.int32),
        act_gear=np.array([float(a.get("gear", 1)) for a in acts]),
        act_kp=np.array([float(a.get("kp", 1)) for a in acts]),
        act_ctrlrange=np.array([_act_range(a, "ctrlrange", "ctrllimited") for a in acts], dtype=np.float64).reshape(-1, 2),
        act_forcerange=np.array([_act_range(a, "forcerange", "forcelimited") for a in acts], dtype=np.float64).reshape(-1, 2))


def buffer_caps(nv: int):
    """-> (nconmax, njmax).  Device-friendly buffer caps (the XML asks for nconmax=100 njmax=500, world.xml:44, which MuJoCo only
    uses as buffer sizes): contacts beyond nconmax / rows beyond njmax are dropped identically by the
    oracle and the HIP path.  One lane group (16 or 32 lanes) serves an env, so caps are multiples of it."""
    group = 16 if nv <= 16 else 32
    eff_nconmax = group
    # 32-lane models: 124 rows - measured on cfg4 (8192 envs x 300 env-steps of the bench: 7.4e8 env-substeps) 3.1e5 substeps wanted 97-104 rows,
    # 8.9e3 105-112, 1.4e3 113-120, 24 121-128, 1 more: with 124 fewer than 4e-8 of the env-substeps drop a row (96 rows: 4.3e-4); 124 is what
    # the 20 KB of LDS per workgroup hold once the pair / geom tables are read from global memory (persist.h: TG)
    eff_njmax = {True: 48, False: 124}[nv <= 16]
    return eff_nconmax, eff_njmax


def _link_dofmask(lk: _Link, dofs: List[_Dof]) -> int:
    """bit k is set when dof k lies on the path from the link to the root"""
    mask, k = 0, lk.dofadr + lk.dofnum - 1
    while k >= 0:
        mask |= (1 << k)
        k = dofs[k].parent
    return mask


def assemble_arrays(bodies, fold: _Fold, dofs: List[_Dof], qpos0, geoms: List[_CollGeom], mesh_vert, pairs: List[_Pair], slot,
                    act: Dict[str, np.ndarray], opt: dict) -> Dict[str, np.ndarray]:
    """The blob's tables (model.py: _ARRAY_FIELDS), one comprehension per field; the qpos0 statistics are filled in afterwards."""
    links, nv, ngeom, npair = fold.links, len(dofs), len(geoms), len(pairs)
    i32 = dict(dtype=np.int32)
    arrays = dict(
        qpos0=np.array(qpos0),
        link_dofmask=np.array([_link_dofmask(lk, dofs) for lk in links], **i32),
        link_parent=np.array([lk.parent for lk in links], **i32),
        link_pos=np.array([lk.pos for lk in links]), link_quat=np.array([lk.quat for lk in links]),
        link_dofadr=np.array([lk.dofadr for lk in links], **i32), link_dofnum=np.array([lk.dofnum for lk in links], **i32),
        link_qposadr=np.array([lk.qposadr for lk in links], **i32), link_free=np.array([lk.free for lk in links], **i32),
        link_mass=np.array([lk.inertial.mass for lk in links], dtype=np.float64), link_com=np.array([lk.inertial.com for lk in links]),
        link_inertia=np.array([[I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]] for I in (lk.inertial.inertia for lk in links)]),
        dof_link=np.array([d.link for d in dofs], **i32), dof_type=np.array([d.type for d in dofs], **i32),
        dof_axis=np.array([d.axis for d in dofs]).reshape(nv, 3), dof_pos=np.array([d.pos for d in dofs]).reshape(nv, 3),
        dof_parent=np.array([d.parent for d in dofs], **i32), dof_damping=np.array([d.damping for d in dofs]),
        dof_qposadr=np.array([d.qposadr for d in dofs], **i32),
        dof_invweight0=np.zeros(nv), dof_limited=np.array([d.limited for d in dofs], **i32),
        dof_range=np.array([d.range for d in dofs]).reshape(nv, 2),
        dof_solref=np.tile([0.02, 1.0], (nv, 1)), dof_solimp=np.tile([0.9, 0.95, 0.001, 0.5, 2.0], (nv, 1)),
        body_link=fold.body_link, body_pos=fold.body_pos, body_quat=fold.body_quat,
        body_mocap=np.array([int(b.mocap) for b in bodies], **i32),
        geom_type=np.array([g.geom.type for g in geoms], **i32),
        geom_link=np.array([g.link for g in geoms], **i32),
        geom_body=np.array([g.body for g in geoms], **i32),
        geom_pos=np.array([g.pos for g in geoms]), geom_quat=np.array([g.quat for g in geoms]),
        geom_size=np.array([g.shape.size for g in geoms]), geom_rbound=np.array([g.shape.rbound for g in geoms]),
        geom_condim=np.array([g.geom.condim for g in geoms], **i32),
        geom_meshadr=np.array([g.meshadr for g in geoms], **i32),
        geom_meshnum=np.array([g.meshnum for g in geoms], **i32),
        geom_invweight=np.zeros((ngeom, 2)),
        geom_aabb=np.array([g.shape.aabb for g in geoms]).reshape(ngeom, 6),
        mesh_vert=mesh_vert,
        pair_geom1=np.array([p.g1 for p in pairs], **i32),
        pair_geom2=np.array([p.g2 for p in pairs], **i32),
        pair_fn=np.array([p.fn for p in pairs], **i32),
        pair_condim=np.array([p.condim for p in pairs], **i32),
        pair_slot=slot,
        pair_friction=np.array([p.friction for p in pairs]).reshape(npair, 5),
        pair_solref=np.array([p.solref for p in pairs]).reshape(npair, 2),
        pair_solimp=np.array([p.solimp for p in pairs]).reshape(npair, 5),
        **act,
    )
    sizes = np.zeros(16, dtype=np.int32)
    sizes[[SZ_NQ, SZ_NV, SZ_NU, SZ_NLINK, SZ_NBODY, SZ_NGEOM, SZ_NPAIR, SZ_NMESHVERT, SZ_NSLOT,
           SZ_NLIMIT, SZ_NCONMAX, SZ_NJMAX, SZ_NMOCAP]] = [
        len(qpos0), nv, len(act["act_dof"]), len(links), len(bodies), ngeom, npair, len(mesh_vert), slot[-1],
        sum(d.limited for d in dofs), opt["nconmax"], opt["njmax"], sum(b.mocap for b in bodies)]
    optv = np.zeros(16)
    optv[[OPT_TIMESTEP, OPT_IMPRATIO, OPT_GRAV_Z, OPT_TOLERANCE, OPT_ITERATIONS, OPT_LS_ITERATIONS,
          OPT_LS_TOLERANCE, OPT_MPR_TOLERANCE, OPT_MPR_ITERATIONS]] = [
        opt["timestep"], opt["impratio"], -9.81, 1e-8, 100, 50, 0.01, 1e-6, 50]
    arrays["sizes"], arrays["opt"] = sizes, optv
    return arrays


def _count_dense_dofs(model: Model) -> int:
    """dofs >= ndense never couple to another dof in M (e.g. a free box with its COM at the body origin):
    the cooperative Cholesky skips their off-diagonal updates when factoring M and M + h B"""
    rs = np.random.default_rng(0)
    dense = 0
    for _ in range(4):
        qr = model.qpos0.copy()
        qr[:model.nu] += rs.uniform(-0.3, 0.3, model.nu)
        for l in range(1, model.nlink):
            if model.link_free[l]:
                a = model.link_qposadr[l]
                qr[a + 3:a + 7] = quat_normalize(rs.normal(size=4))
        Mr = mass_matrix(model, qr)
        off = np.abs(Mr - np.diag(np.diag(Mr))) > 1e-12
        idx = np.where(off.any(axis=0))[0]
        dense = max(dense, int(idx.max()) + 1 if idx.size else 0)
    return dense


def _body_invweights(model: Model, Minv, inertials: List[_MassProps]) -> np.ndarray:
    """Per body (translational, rotational): mean diagonal of J M^-1 J^T at the body's centre of mass, at qpos0."""
    xpos, xquat = link_kinematics(model, model.qpos0)
    ang, lin, anchor = dof_motion(model, xpos, xquat, model.qpos0)
    body_invw = np.zeros((model.nbody, 2))
    for i in range(1, model.nbody):
        l = model.body_link[i]
        if l == 0:
            continue
        Rl = quat_to_mat(xquat[l])
        c = xpos[l] + Rl @ (model.body_pos[i] + quat_to_mat(model.body_quat[i]) @ inertials[i].com)
        jp, jr = point_jacobian(model, ang, lin, anchor, l, c)
        body_invw[i, 0] = np.trace(jp @ Minv @ jp.T) / 3.0
        body_invw[i, 1] = np.trace(jr @ Minv @ jr.T) / 3.0
    return body_invw


def fill_qpos0_statistics(model: Model, inertials: List[_MassProps]):
    """mj_setConst: meaninertia, dof and body inverse weights at qpos0 (used by the constraint regulariser), and ndense."""
    M0 = mass_matrix(model, model.qpos0)
    Minv = np.linalg.inv(M0)
    model.opt[OPT_MEANINERTIA] = np.trace(M0) / model.nv
    dinv = np.diag(Minv).copy()
    for l in range(1, model.nlink):
        if model.link_free[l]:
            a = model.link_dofadr[l]
            dinv[a:a + 3] = dinv[a:a + 3].mean(); dinv[a + 3:a + 6] = dinv[a + 3:a + 6].mean()
    model.dof_invweight0[:] = dinv
    model.sizes[SZ_NDENSE] = _count_dense_dofs(model)
    body_invw = _body_invweights(model, Minv, inertials)
    model.geom_invweight[:] = body_invw[model.geom_body]
    model.meta["body_invweight0"] = body_invw.tolist()
    model.meta["link_mass"] = model.link_mass.tolist()


def compile_model(dofs: Sequence[str] = ("slide_x", "slide_y"), n_blocks: int = 0,
                  block_pos: Optional[np.ndarray] = None, xml_file: str = "models/world.xml",
                  ref_root: Path = DEFAULT_REF_ROOT, set_xml: Sequence = (), block_geom: Optional[dict] = None,
                  plane_convex_points: int = 1) -> Model:
    """plane_convex_points: contacts a plane <-> convex (mesh / cylinder) pair may hold - 1: the deepest support point only (the committed
    reference configurations); 4: up to three more around it, as MuJoCo's mjc_PlaneConvex adds them (oracle/hsr_oracle.c)."""
    assert plane_convex_points in (1, 4)
    xml_path = Path(ref_root) / xml_file
    set_xml = [(str(p), str(v)) for p, v in set_xml]
    root, acts = _mutated_tree(xml_path, list(dofs), _block_positions(block_pos, n_blocks), set_xml, block_geom)
    parsed = _read_tree(root, xml_path)
    bodies, opt, meta = parsed.bodies, parsed.opt, parsed.meta
    if set_xml:
        meta.update(set_xml=[list(c) for c in set_xml])
    meta.update(plane_convex_points=int(plane_convex_points))
    if block_geom:
        meta.update(block_geom=dict(block_geom))
    meta.update(dofs=list(dofs), n_blocks=n_blocks, xml_file=xml_file,
                decisions="H1 malformed pos->0; H2 inertiafromgeom all geoms density 1000 (legacy "
                          "mesh inertia); H3 default class 'all' is global; H4 hinge ranges in "
                          "degrees; H5 quats normalised; H6 goal is mocap; H7 MuJoCo 2.0 defaults")

    meshes = _MeshCache(parsed.meshes)
    inertials = body_inertias(bodies, parsed.inertiafromgeom, meshes)
    fold = fold_links(bodies, inertials)
    dof_recs, qpos0, joints = assign_dofs(bodies, fold.links)
    geoms, mesh_vert = collidable_geoms(bodies, fold, meshes)
    pairs = candidate_pairs(geoms, fold.links, bodies, parsed.excludes)
    slot = pair_slots(pairs, plane_convex_points)
    act = actuator_tables(acts, joints)
    meta["xml_nconmax_njmax"] = [opt["nconmax"], opt["njmax"]]
    opt["nconmax"], opt["njmax"] = buffer_caps(len(dof_recs))
    assert opt["cone"] == "elliptic", "only the reference's elliptic cones are implemented"
    arrays = assemble_arrays(bodies, fold, dof_recs, qpos0, geoms, mesh_vert, pairs, slot, act, opt)

    names = dict(body=[b.name for b in bodies], joint=[j.name for j in joints], geom=[g.name for g in geoms],
                 actuator=[a.get("name") for a in acts],
                 link=[bodies[lk.body].name for lk in fold.links])
    meta["joint_qposadr"] = [(j.qposadr, j.nq) for j in joints]
    meta["joint_dofadr"] = [j.dofadr for j in joints]
    meta["mesh_license"] = ("hull vertices derived from hsr/hsr_meshes (Toyota, CC BY-NC-ND 4.0, "
                            "hsr/hsr_meshes/LICENSE.txt); kept only as collision tables")
    model = Model(arrays=arrays, names=names, meta=meta)
    fill_qpos0_statistics(model, inertials)
    return model


# the four benchmark configurations of BASELINE.json
CONFIGS = {
    "cfg1": dict(dofs=["slide_x", "slide_y"], n_blocks=0),
    "cfg2": dict(dofs=["slide_x", "slide_y"], n_blocks=1),
    "cfg3": dict(dofs=ALL_DOFS, n_blocks=1),
    "cfg4": dict(dofs=ALL_DOFS, n_blocks=3),
    # the cupboard scene (cupboard-world.xml:91-116) with its own `block` / `blockjoint`, the shape of the
    # hsr/__init__.py:10-19 demo; many more box geoms -> 274 candidate pairs
    "cupboard": dict(dofs=ALL_DOFS, n_blocks=0, xml_file="models/cupboard-world.xml"),
}
# further committed blobs, used by the parity tests only (the GPU box has no reference tree to compile from):
#   cfg3_setxml  SURVEY 8f row 2: cfg3 through `--set-xml` (pan friction halved, arm-lift actuator without ctrl limit)
#   nq18         a model whose qpos (18) does not fit the 16 lanes its 16 dofs select: must fall back to the per-substep chain
TEST_CONFIGS = {
    "cfg3_setxml": dict(dofs=ALL_DOFS, n_blocks=1,
                        set_xml=[("worldbody/body[@name='pan']/geom/friction", "0.5 0.005 0.0001"),
                                 ("actuator/position[@name='arm_lift_motor']/ctrllimited", "false")]),
    "nq18": dict(dofs=["slide_x", "slide_y", "arm_lift_joint", "arm_flex_joint"], n_blocks=2),
    # sizes none of the reference configurations has: they run the GENERIC instances of the persistent kernel (nv and ndense at
    # run time) - nv 11 in a 16-lane group, nv 23 in a 32-lane group
    "nv11": dict(dofs=["slide_x", "slide_y", "arm_lift_joint", "arm_flex_joint", "wrist_roll_joint"], n_blocks=1),
    "nv23": dict(dofs=["slide_x", "slide_y", "arm_lift_joint", "arm_flex_joint", "wrist_roll_joint"], n_blocks=3),
    # no robot dof at all: the robot is scenery (15 static hulls + the wrist cylinder), the block the only body - thrown around it, it
    # leaves and re-enters the cull ranges of the hulls (the separation-margin stamps of the convex pairs: tests/test_gpu_hotpath.py)
    "static1": dict(dofs=[], n_blocks=1),
    # plane <-> convex with several points (round 4): the head-pan hull (32 vertices, a flat bottom face of 61 cm^2) as a free body lying on
    # the FLOOR plane, away from the robot; the same scene with the single deepest point for comparison (tests/test_kat.py)
    "meshrest4": dict(dofs=[], n_blocks=1, block_geom=dict(type="mesh", mesh="head_pan"), plane_convex_points=4,
                      block_pos=np.array([[1.0, 0.6, 0.05]])),
    "meshrest1": dict(dofs=[], n_blocks=1, block_geom=dict(type="mesh", mesh="head_pan"), plane_convex_points=1,
                      block_pos=np.array([[1.0, 0.6, 0.05]])),
}


def emit_mjcf(outdir, name: str, dofs: Sequence[str] = ("slide_x", "slide_y"), n_blocks: int = 0,
              block_pos: Optional[np.ndarray] = None, xml_file: str = "models/world.xml",
              ref_root: Path = DEFAULT_REF_ROOT, set_xml: Sequence = (), block_geom: Optional[dict] = None) -> Path:
    """Write the MJCF that the reference's launcher would hand to mujoco-py for this configuration - the mutations of
    hsr/util.py:93-159 (block injection, --set-xml, actuator / joint filter, include and meshdir paths) applied to the
    main file and to every included file - as <outdir>/<name>.xml (+ <name>__<include>).  Anyone with a MuJoCo install
    can load it to generate external golden vectors (tests/test_mujoco_crosscheck.py)."""
    ref_root, outdir = Path(ref_root), Path(outdir)
    outdir.mkdir(parents=True, exist_ok=True)
    xml_path = ref_root / xml_file
    block_pos = _block_positions(block_pos, n_blocks)
    set_xml = [(str(p), str(v)) for p, v in set_xml]
    includes = [e.get("file") for e in ET.parse(xml_path).findall("*/include")]
    out_main = outdir / f"{name}.xml"
    for rel in [None] + includes:
        src = xml_path if rel is None else xml_path.parent / rel
        tree = ET.parse(src)
        root = tree.getroot()
        worldbody = root.find("./worldbody")
        if worldbody is not None:
            _inject_blocks(worldbody, block_pos, block_geom)
        _apply_setters(root, set_xml)
        _filter_dofs(root, dofs)
        for inc in root.findall("*/include"):
            inc.set("file", f"{name}__{Path(inc.get('file')).name}")
        for comp in root.findall("compiler"):
            comp.set("meshdir", str((xml_path.parent / comp.get("meshdir", ".")).resolve()))
        tree.write(out_main if rel is None else outdir / f"{name}__{Path(rel).name}")
    return out_main


def main():
    import argparse
    ap = argparse.ArgumentParser(description="compile the committed model blobs / emit the mutated MJCF of each configuration")
    ap.add_argument("--emit-mjcf", metavar="DIR", default=None,
                    help="write <DIR>/<config>.xml (what hsr/util.py:mutate_xml yields) for every configuration instead of compiling")
    args = ap.parse_args()
    every = dict(CONFIGS, **TEST_CONFIGS)
    if args.emit_mjcf:
        for name, kw in every.items():
            print(emit_mjcf(args.emit_mjcf, name, **{k: v for k, v in kw.items() if k != "plane_convex_points"}))  # not an XML property
        return
    MODEL_DIR.mkdir(exist_ok=True)
    for name, kw in every.items():
        m = compile_model(**kw)
        m.save(MODEL_DIR / f"{name}.hsrm")
        print(name, "nq", m.nq, "nv", m.nv, "nu", m.nu, "nlink", m.nlink, "nbody", m.nbody,
              "ngeom", m.ngeom, "npair", m.npair, "nslot", m.nslot, "bytes", len(m.to_bytes()))


if __name__ == "__main__":
    main()
