"""The compiled model ("model blob"): container, table layout and the fp64 numpy reference of the kinematics and mass matrix.

What the run time needs - env.py, sim.py, render.py, the benchmark, the tests and tools load the blobs committed under
``models/`` and read them through ``Model``.  Producing a blob from the MJCF / STL data files is compiler.py's job.
"""
from __future__ import annotations

import json
import struct
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List

import numpy as np

# MuJoCo geom type enum values (kept so tables read like mjModel)
GEOM_PLANE, GEOM_SPHERE, GEOM_CYLINDER, GEOM_BOX, GEOM_MESH = 0, 2, 5, 6, 7
# dof types
DOF_SLIDE, DOF_HINGE, DOF_FREE_LIN, DOF_FREE_ANG = 0, 1, 2, 3
# narrowphase function per candidate pair
FN_PLANE_BOX, FN_PLANE_CONVEX, FN_BOX_BOX, FN_CONVEX = 0, 1, 2, 3
UNLIMITED = 1e30     # range of an actuator without ctrllimited / forcelimited (finite in fp32)
FN_MAXCON = {FN_PLANE_BOX: 4, FN_PLANE_CONVEX: 1, FN_BOX_BOX: 8, FN_CONVEX: 1}

BLOB_MAGIC = b"HSRM0001"
MODEL_DIR = Path(__file__).parent / "models"


# ----------------------------------------------------------------------------- math helpers
def quat_normalize(q):
    q = np.asarray(q, dtype=np.float64)
    return q / np.linalg.norm(q)


def quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz,
                     aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw])


def quat_to_mat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def axis_angle_quat(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    s = np.sin(0.5 * angle)
    return np.array([np.cos(0.5 * angle), axis[0] * s, axis[1] * s, axis[2] * s])


# ----------------------------------------------------------------------------- the model
_ARRAY_FIELDS = [
    # scalars packed as arrays for a uniform container
    "sizes", "opt",
    "qpos0",
    "link_parent", "link_pos", "link_quat", "link_dofadr", "link_dofnum", "link_qposadr",
    "link_free", "link_mass", "link_com", "link_inertia", "link_dofmask",
    "dof_link", "dof_type", "dof_axis", "dof_pos", "dof_parent", "dof_damping", "dof_qposadr",
    "dof_invweight0", "dof_limited", "dof_range", "dof_solref", "dof_solimp",
    "body_link", "body_pos", "body_quat", "body_mocap",
    "geom_type", "geom_link", "geom_body", "geom_pos", "geom_quat", "geom_size", "geom_rbound",
    "geom_condim", "geom_meshadr", "geom_meshnum", "geom_invweight", "geom_aabb",
    "mesh_vert",
    "pair_geom1", "pair_geom2", "pair_fn", "pair_condim", "pair_slot", "pair_friction",
    "pair_solref", "pair_solimp",
    "act_dof", "act_gear", "act_kp", "act_ctrlrange", "act_forcerange",
]

# index constants into ``sizes`` / ``opt`` (mirrored in include/hsrsim.h and oracle/hsr_oracle.c)
SZ_NQ, SZ_NV, SZ_NU, SZ_NLINK, SZ_NBODY, SZ_NGEOM, SZ_NPAIR, SZ_NMESHVERT, SZ_NSLOT, \
    SZ_NLIMIT, SZ_NCONMAX, SZ_NJMAX, SZ_NMOCAP, SZ_NDENSE = range(14)
OPT_TIMESTEP, OPT_IMPRATIO, OPT_GRAV_Z, OPT_TOLERANCE, OPT_ITERATIONS, OPT_LS_ITERATIONS, \
    OPT_LS_TOLERANCE, OPT_MPR_TOLERANCE, OPT_MPR_ITERATIONS, OPT_MEANINERTIA = range(10)


@dataclass
class Model:
    arrays: Dict[str, np.ndarray]
    names: Dict[str, List[str]]
    meta: Dict[str, object]

    def __getattr__(self, k):
        arrays = object.__getattribute__(self, "arrays")
        if k in arrays:
            return arrays[k]
        raise AttributeError(k)

    # -- sizes
    @property
    def nq(self): return int(self.arrays["sizes"][SZ_NQ])
    @property
    def nv(self): return int(self.arrays["sizes"][SZ_NV])
    @property
    def nu(self): return int(self.arrays["sizes"][SZ_NU])
    @property
    def nlink(self): return int(self.arrays["sizes"][SZ_NLINK])
    @property
    def nbody(self): return int(self.arrays["sizes"][SZ_NBODY])
    @property
    def ngeom(self): return int(self.arrays["sizes"][SZ_NGEOM])
    @property
    def npair(self): return int(self.arrays["sizes"][SZ_NPAIR])
    @property
    def nslot(self): return int(self.arrays["sizes"][SZ_NSLOT])
    @property
    def timestep(self): return float(self.arrays["opt"][OPT_TIMESTEP])

    def body_id(self, name: str) -> int:
        return self.names["body"].index(name)

    def scalar_joints(self):
        """(qpos addresses, dof addresses) of the 1-dof joints (the robot), in joint order; scenes differ in whether the
        block's free joint comes before (cupboard-world.xml) or after (world.xml + util.py injection) the robot."""
        qa = [a for (a, n) in self.meta["joint_qposadr"] if n == 1]
        da = [d for (a, n), d in zip(self.meta["joint_qposadr"], self.meta["joint_dofadr"]) if n == 1]
        return np.array(qa, dtype=int), np.array(da, dtype=int)

    def free_joint_qadrs(self):
        """qpos start address of every free joint (x y z qw qx qy qz), in joint order."""
        return [a for (a, n) in self.meta["joint_qposadr"] if n == 7]

    def block_body(self) -> str:
        """Name of the first free body: `block0` (util.py:109) or `block` (cupboard-world.xml:113)."""
        for cand in ("block0", "block"):
            if cand in self.names["body"]:
                return cand
        return ""

    def joint_qpos_addr(self, name: str):
        """mujoco_py ``model.get_joint_qpos_addr`` (reference use: hsr/env.py:153)."""
        j = self.names["joint"].index(name)
        adr, n = self.meta["joint_qposadr"][j]
        return adr if n == 1 else (adr, adr + n)

    # -- (de)serialisation ------------------------------------------------------------------
    def to_bytes(self) -> bytes:
        """Container: magic | u32 n | n x (name[32], u32 dtype, u32 ndim, u32 shape[4], u64 off,
        u64 nbytes) | json_len u64 | json | data (8-byte aligned).  dtype 0=f64, 1=i32."""
        entries, blobs, off = [], [], 0
        for name in _ARRAY_FIELDS:
            a = self.arrays[name]
            if a.dtype.kind == "f":
                a = np.ascontiguousarray(a, dtype="<f8"); code = 0
            else:
                a = np.ascontiguousarray(a, dtype="<i4"); code = 1
            shape = list(a.shape) + [0] * (4 - a.ndim)
            raw = a.tobytes()
            pad = (-len(raw)) % 8
            entries.append(struct.pack("<32sII4IQQ", name.encode(), code, a.ndim, *shape, off, len(raw)))
            blobs.append(raw + b"\0" * pad)
            off += len(raw) + pad
        js = json.dumps(dict(names=self.names, meta=self.meta)).encode()
        js += b" " * ((-len(js)) % 8)
        head = BLOB_MAGIC + struct.pack("<I", len(entries)) + b"\0" * 4
        return head + b"".join(entries) + struct.pack("<Q", len(js)) + js + b"".join(blobs)

    @staticmethod
    def from_bytes(raw: bytes) -> "Model":
        assert raw[:8] == BLOB_MAGIC, "not an HSRM blob"
        n = struct.unpack("<I", raw[8:12])[0]
        p = 16
        ents = []
        esz = struct.calcsize("<32sII4IQQ")
        for _ in range(n):
            ents.append(struct.unpack("<32sII4IQQ", raw[p:p + esz])); p += esz
        jl = struct.unpack("<Q", raw[p:p + 8])[0]; p += 8
        js = json.loads(raw[p:p + jl].decode()); p += jl
        arrays = {}
        for name, code, ndim, s0, s1, s2, s3, off, nb in ents:
            shape = (s0, s1, s2, s3)[:ndim]
            dt = "<f8" if code == 0 else "<i4"
            arrays[name.rstrip(b"\0").decode()] = np.frombuffer(
                raw, dtype=dt, count=nb // (8 if code == 0 else 4), offset=p + off).reshape(shape).copy()
        return Model(arrays=arrays, names=js["names"], meta=js["meta"])

    def save(self, path):
        Path(path).write_bytes(self.to_bytes())

    @staticmethod
    def load(path) -> "Model":
        return Model.from_bytes(Path(path).read_bytes())


# ----------------------------------------------------------------------------- numpy reference
def link_kinematics(m: Model, qpos: np.ndarray):
    """fp64 forward kinematics over links -> (xpos[nlink,3], xquat[nlink,4]).

    Restates mj_kinematics for the folded tree: body frame = parent * (pos, quat); joints of a
    body applied in order (slide: translate along the current axis; hinge: rotate about the
    anchor); free joint: pose read from qpos with the quaternion normalised.
    """
    nl = m.nlink
    xpos = np.zeros((nl, 3)); xquat = np.zeros((nl, 4)); xquat[0, 0] = 1
    for l in range(1, nl):
        if m.link_free[l]:
            a = m.link_qposadr[l]
            xpos[l] = qpos[a:a + 3]
            xquat[l] = quat_normalize(qpos[a + 3:a + 7])
            continue
        p = m.link_parent[l]
        R = quat_to_mat(xquat[p])
        pos = xpos[p] + R @ m.link_pos[l]
        quat = quat_mul(xquat[p], m.link_quat[l])
        for d in range(m.link_dofadr[l], m.link_dofadr[l] + m.link_dofnum[l]):
            q = qpos[m.dof_qposadr[d]]
            Rl = quat_to_mat(quat)
            if m.dof_type[d] == DOF_SLIDE:
                pos = pos + Rl @ m.dof_axis[d] * q
            else:
                anchor = pos + Rl @ m.dof_pos[d]
                quat = quat_mul(quat, axis_angle_quat(m.dof_axis[d], q))
                pos = anchor - quat_to_mat(quat) @ m.dof_pos[d]
        xpos[l], xquat[l] = pos, quat_normalize(quat)
    return xpos, xquat


def dof_motion(m: Model, xpos, xquat, qpos):
    """World-frame motion axes: for each dof (ang[3], lin-axis[3], anchor[3])."""
    nv = m.nv
    ang = np.zeros((nv, 3)); lin = np.zeros((nv, 3)); anchor = np.zeros((nv, 3))
    for l in range(1, m.nlink):
        R = quat_to_mat(xquat[l])
        if m.link_free[l]:
            d0 = m.link_dofadr[l]
            for k in range(3):
                lin[d0 + k, k] = 1.0
                ang[d0 + 3 + k] = R[:, k]
                anchor[d0 + 3 + k] = xpos[l]
            continue
        # joints applied in order: axis of joint d is expressed in the frame *after* earlier
        # joints of the same body; for this model a body never mixes hinges (all slides or one
        # hinge), so the final link frame gives the same axes.
        for d in range(m.link_dofadr[l], m.link_dofadr[l] + m.link_dofnum[l]):
            ax = R @ m.dof_axis[d]
            if m.dof_type[d] == DOF_SLIDE:
                lin[d] = ax
            else:
                ang[d] = ax
                anchor[d] = xpos[l] + R @ m.dof_pos[d]
    return ang, lin, anchor


def point_jacobian(m: Model, ang, lin, anchor, link: int, point):
    """jacp[3,nv], jacr[3,nv] of a world point rigidly attached to ``link``."""
    jp = np.zeros((3, m.nv)); jr = np.zeros((3, m.nv))
    if link == 0:
        return jp, jr
    d = m.link_dofadr[link] + m.link_dofnum[link] - 1
    while d >= 0:
        jr[:, d] = ang[d]
        jp[:, d] = lin[d] + np.cross(ang[d], point - anchor[d])
        d = m.dof_parent[d]
    return jp, jr


def mass_matrix(m: Model, qpos):
    xpos, xquat = link_kinematics(m, qpos)
    ang, lin, anchor = dof_motion(m, xpos, xquat, qpos)
    M = np.zeros((m.nv, m.nv))
    for l in range(1, m.nlink):
        R = quat_to_mat(xquat[l])
        c = xpos[l] + R @ m.link_com[l]
        ixx, iyy, izz, ixy, ixz, iyz = m.link_inertia[l]
        I = R @ np.array([[ixx, ixy, ixz], [ixy, iyy, iyz], [ixz, iyz, izz]]) @ R.T
        jp, jr = point_jacobian(m, ang, lin, anchor, l, c)
        M += m.link_mass[l] * jp.T @ jp + jr.T @ I @ jr
    return M


def load_config(name: str) -> Model:
    """Load a committed blob (no reference tree needed)."""
    return Model.load(MODEL_DIR / f"{name}.hsrm")
