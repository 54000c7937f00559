"""External pin of the oracle: when a real MuJoCo is importable (`mujoco`, or the reference's own
`mujoco_py`) AND the reference's data files are on disk (tests/golden/hsr_data), the MJCF that hsr/util.py:mutate_xml would produce for each
configuration (hsr_env_amd.compiler.emit_mjcf) is loaded into it, the golden rollouts' inputs are replayed, and the oracle's
committed trajectories must follow MuJoCo's per substep.  Neither is available in the build container or on the GPU box, so this
file normally SKIPS; run it wherever MuJoCo lives, with HSR_WRITE_MUJOCO_GOLDEN=1 to also write tests/golden/mujoco_<cfg>.npz,
which tests/test_golden.py then prefers as the pin.  Until such fixtures exist parity with mujoco-py stays UNPINNED.

Stated tolerance (fp64 oracle vs fp64 MuJoCo, same MJCF, same inputs): |dqpos| < 1e-6 and |dqvel| < 1e-4 (1 + |qvel|) per substep
while the contact sets agree; the engine version is recorded in the fixture (the reference pins none: setup.py:26)."""
import os
from pathlib import Path

import numpy as np
import pytest

from hsr_env_amd import compiler as hc

GOLD = Path(__file__).parent / "golden"
REF_DATA = GOLD / "hsr_data"          # the reference's MJCF scenes and STL meshes, stored verbatim


def _engine():
    try:
        import mujoco
        return "mujoco", mujoco
    except ImportError:
        pass
    try:
        import mujoco_py
        return "mujoco_py", mujoco_py
    except ImportError:
        return None, None


KIND, ENGINE = _engine()
pytestmark = [pytest.mark.skipif(ENGINE is None, reason="no MuJoCo (mujoco / mujoco_py) importable"),
              pytest.mark.skipif(not REF_DATA.exists(), reason="reference MJCF / STL data files not on disk")]


def _rollout(xml, names, q0, ctrl, nsub):
    """per-env trajectories (qpos, qvel, ncon) of the engine; joints matched to the compiled model by name"""
    if KIND == "mujoco":
        model = ENGINE.MjModel.from_xml_path(str(xml))
        data = ENGINE.MjData(model)
        qadr = [int(model.joint(n).qposadr[0]) for n in names]; vadr = [int(model.joint(n).dofadr[0]) for n in names]
        step = lambda: ENGINE.mj_step(model, data)
        reset = lambda: ENGINE.mj_resetData(model, data)
        version = ENGINE.__version__
    else:
        model = ENGINE.load_model_from_path(str(xml))
        sim = ENGINE.MjSim(model)
        data = sim.data
        adr = [model.get_joint_qpos_addr(n) for n in names]; qadr = [a if isinstance(a, (int, np.integer)) else a[0] for a in adr]
        adr = [model.get_joint_qvel_addr(n) for n in names]; vadr = [a if isinstance(a, (int, np.integer)) else a[0] for a in adr]
        step, reset, version = sim.step, sim.reset, getattr(ENGINE, "__version__", "mujoco_py")
    order_q = np.argsort(qadr); order_v = np.argsort(vadr)
    assert list(order_q) == list(range(len(names))) and list(order_v) == list(range(len(names))), "joint order differs from the compiled model"
    ne = q0.shape[0]
    Q = np.zeros((ne, nsub, q0.shape[1])); V = np.zeros((ne, nsub, model.nv)); C = np.zeros((ne, nsub), np.int32)
    for e in range(ne):
        reset()
        data.qpos[:] = q0[e]; data.ctrl[:] = ctrl[e]
        for k in range(nsub):
            step()
            Q[e, k], V[e, k], C[e, k] = data.qpos, data.qvel, data.ncon
    return Q, V, C, version


@pytest.mark.parametrize("cfg", ["cfg1", "cfg2", "cfg3", "cfg4", "cupboard"])
def test_oracle_follows_mujoco(models, cfg, tmp_path):
    g = np.load(GOLD / f"golden_{cfg}.npz")
    m = models[cfg]
    kw = dict(hc.CONFIGS[cfg])
    xml = hc.emit_mjcf(tmp_path, cfg, ref_root=REF_DATA, **kw)
    names = [n for n in m.names["joint"] if n]
    nsub = g["qpos"].shape[1]
    Q, V, C, version = _rollout(xml, names, g["qpos0"], g["ctrl"], nsub)
    if os.environ.get("HSR_WRITE_MUJOCO_GOLDEN") == "1":
        np.savez_compressed(GOLD / f"mujoco_{cfg}.npz", qpos0=g["qpos0"], ctrl=g["ctrl"], qpos=Q, qvel=V, ncon=C, engine=f"{KIND} {version}")
    same = C == g["ncon"]
    dq = np.abs(Q - g["qpos"]).max(-1); dv = (np.abs(V - g["qvel"]) / (1 + np.abs(V))).max(-1)
    # compare up to the first substep at which the contact sets differ (afterwards the trajectories legitimately part)
    upto = np.where(same.all(1), nsub, np.argmin(same, 1))
    bad = [(e, int(upto[e]), float(dq[e, :upto[e]].max(initial=0)), float(dv[e, :upto[e]].max(initial=0))) for e in range(Q.shape[0])
           if upto[e] and (dq[e, :upto[e]].max(initial=0) >= 1e-6 or dv[e, :upto[e]].max(initial=0) >= 1e-4)]
    print(f"{cfg} vs {KIND} {version}: contact sets agree on {same.mean():.1%} of the substeps; {len(bad)} envs outside tolerance")
    assert not bad, bad[:5]
