"""The velocity-dependent smooth dynamics of the device at speed, on every kernel path, against fp64: link velocity recursion, Coriolis and
centrifugal bias of the arm, gyroscopic bias w x I w of a free body, implicit joint damping, free-joint quaternion integration at a general
attitude, link rotation matrices.  The code exists three times:
    const    csrc/kin3.h, straight-line code on the compile-time tree (kernel_flags() == 7): cfg1-4, cupboard
    generic  csrc/kin2.h + the inertia phase of solve_body.inc, table-driven (kernel_flags() == 1): nv11, nv23, any model under HSR_NO_CONST=1
    chain    kin_link_pose / kin_link_dyn / k_kinematics of csrc/collide.h (kernel_flags() == 0): forward(), nq18, set_persistent(False)
States: tests/smooth_ref.py (fast_free_states: the arm at up to 2 rad/s, blocks tumbling at up to 8 rad/s at random attitudes, no contact and no
active limit for 50 substeps in both oracle builds), 50 envs so that the last wave is partly filled.  Every comparison with the fp64 oracle is
held to 8 x what the fp32 build of the oracle leaves of the same quantity on the same states (smooth_ref.compare; never derived from a kernel),
prints floor, bound, distance and magnitude, and asserts that the bound is at most 1e-3 of the quantity's median magnitude."""
import numpy as np
import pytest

import smooth_ref as sr
from hsr_env_amd import sim as hs

pytestmark = pytest.mark.gpu

N = 50
NSUB = 50
PATHS = [("const", "cfg1"), ("const", "cfg2"), ("const", "cfg3"), ("const", "cfg4"), ("const", "cupboard"),
         ("generic", "nv11"), ("generic", "nv23"), ("generic", "cfg3"), ("generic", "cfg4"),
         ("chain", "nq18"), ("chain", "cfg3")]
FLAGS = {"const": 7, "generic": 1, "chain": 0}


def open_sim(models, path, cfg, monkeypatch):
    """A batch of N envs of `cfg` on kernel path `path`, the path asserted through kernel_flags()."""
    m = models[cfg]
    monkeypatch.setenv("HSR_NO_CONST", "1" if path == "generic" else "0")
    sim = hs.BatchSim(m, N)
    if path == "chain" and sim.is_persistent():
        assert sim.set_persistent(False) is False
    assert sim.kernel_flags() == FLAGS[path], (path, cfg, sim.kernel_flags())
    return m, sim


def assert_contact_free(sim, what):
    """F_NCON / F_NEFC of every env's last substep (the persistent kernel stores them under set_debug, the chain always): a non-zero count fails."""
    ncon, nefc = sim.get_field(hs.F_NCON), sim.get_field(hs.F_NEFC)
    assert not ncon.any() and not nefc.any(), f"{what}: envs with contacts {np.flatnonzero(ncon).tolist()}, with constraint rows {np.flatnonzero(nefc).tolist()}"


def one_substep(sim, ref, sign=1.0):
    """set_debug; set_state(q, sign v); step(ctrl, 1) -> (obs, acceleration (v1 - v0) / dt from the returned obs)."""
    m = sim.model
    sim.set_debug(True)
    sim.set_state(np.zeros(N), ref["q"], sign * ref["v"])
    obs, rew, done, ns = sim.step(ref["ctrl"], 1)
    assert (ns == 1).all() and not done.any() and not sim.bad_state()[1]
    assert_contact_free(sim, f"one substep from (q, {sign:+g} v)")
    return obs.astype(np.float64), (obs[:, m.nq:].astype(np.float64) - sign * ref["v"]) / m.timestep


@pytest.mark.parametrize("cfg", ["cfg3", "cfg4", "cupboard", "nq18"])
def test_forward_stages_at_speed(models, cfg):
    """(a) The chain kernels behind forward(): set_state; step(ctrl, 0) to load ctrl; forward().  F_XPOS, F_XMAT, F_M, F_QACC_SMOOTH and
    F_QFRC_SMOOTH against the fp64 oracle's forward pass at the same state, each within its 8 x floor bound; no env has a contact or a
    constraint row."""
    m = models[cfg]
    ref = sr.reference(cfg, m, N, NSUB)
    sim = hs.BatchSim(m, N)
    sim.set_state(np.zeros(N), ref["q"], ref["v"])
    sim.step(ref["ctrl"], 0)
    sim.forward()
    assert_contact_free(sim, "forward()")
    for field, key in ((hs.F_XPOS, "xpos"), (hs.F_XMAT, "xmat"), (hs.F_M, "M"), (hs.F_QACC_SMOOTH, "qacc_smooth"), (hs.F_QFRC_SMOOTH, "qfrc_smooth")):
        sr.compare(f"forward {cfg} {key}", sim.get_field(field), ref["f64"][key], ref["f32"][key])
    sim.close()


@pytest.mark.parametrize("path,cfg", PATHS)
def test_one_substep_at_speed(models, path, cfg, monkeypatch):
    """(b) One substep on every path: the acceleration a = (v1 - v0) / dt taken from the returned obs and the new qpos against the fp64 oracle,
    each within its bound; the quaternion of every block within 4 ulp of unit norm; no contact and no constraint row in any env.
    F_XPOS / F_XMAT after the step are the poses of the forward pass of the LAST substep - of the state that substep started from, here the
    state given to set_state (persist.h stores poseL right after kin3_run / the kin2 stages, before the substep integrates; k_kinematics of
    the chain does the same; the oracle's xpos after step() lags in the same way): they are compared with the oracle's poses at (q, v)."""
    m, sim = open_sim(models, path, cfg, monkeypatch)
    ref = sr.reference(cfg, m, N, NSUB)
    obs, a = one_substep(sim, ref)
    tag = f"substep {path} {cfg}"
    sr.compare(f"{tag} a", a, ref["f64"]["a1"], ref["f32"]["a1"])
    sr.compare(f"{tag} q1", obs[:, :m.nq], ref["f64"]["q1"], ref["f32"]["q1"])
    for adr, d, l in sr.free_joints(m):
        off = np.abs(np.linalg.norm(obs[:, adr + 3:adr + 7], axis=1) - 1).max()
        print(f"{tag}: block at qpos {adr}: | |quat| - 1 | = {off / sr.ULP32:.2f} ulp")
        assert off <= 4 * sr.ULP32
    sr.compare(f"{tag} xpos", sim.get_field(hs.F_XPOS), ref["f64"]["xpos"], ref["f32"]["xpos"])
    sr.compare(f"{tag} xmat", sim.get_field(hs.F_XMAT), ref["f64"]["xmat"], ref["f32"]["xmat"])
    sim.close()


# (c): the share of the median magnitude that the bound on the scalar dofs may reach.  The construction reads the acceleration off the fp32
# velocity that the step returns: v1 is resolved to half an ulp of |v| <= 2, 1.2e-7, so a to 6e-5 whatever computes it, and (M + dt D) carries
# the base's 278 kg: 8e-3 N in the fp32 build of the oracle (measured on the CPU: 6.7e-3 .. 8.6e-3 on the six models with an arm, against a
# median largest component of C of 1.1 .. 2.6), 8 x that is 2.5 % .. 5 % of C.  The 1e-3 of the other comparisons cannot hold for this
# quantity in any implementation; a dropped or mis-signed term is 100 % or 200 % of itself, so a tenth still separates (and (a), (b) and (d)
# see the same terms at 1e-5 of their quantities).  The blocks' angular rows (inertia 1e-3 kg m^2) keep the 1e-3.
INTEGRATOR_GUARD = 0.1


@pytest.mark.parametrize("path,cfg", PATHS)
def test_bias_force_through_the_integrator(models, path, cfg, monkeypatch):
    """(c) The velocity-quadratic bias force on every path, independent of the oracle: three one-substep runs from (q, 0), (q, v), (q, -v);
    the even part of a, a(q,0) - (a(q,v) + a(q,-v)) / 2, times M(q) + dt diag(dof_damping) built in fp64 numpy from model.mass_matrix, must
    equal the Lagrangian bias on the scalar dofs (central differences of the numpy mass matrix) and w x I w on every block's angular dofs
    (zero on its linear dofs).  How the damping enters is restated from solve_body.inc, phase G, contact-free branch: (M + dt D) a = qfrc_smooth,
    v1 = v0 + dt a; damping and the actuators are affine in v and cancel in the even part, gravity is constant.  The oracle only sizes the
    bound - 8 x what its fp32 build leaves of the same three-run construction - and is never the expected value.  cfg1 (two orthogonal slides,
    no block) has no such force: the expected value is zero, still within the bound."""
    m, sim = open_sim(models, path, cfg, monkeypatch)
    ref = sr.reference(cfg, m, N, NSUB)
    a3 = np.stack([one_substep(sim, ref, sign)[1] for sign in (0.0, 1.0, -1.0)], axis=1)
    got, twin, C = sr.bias_through_integrator(ref["A"], a3), sr.bias_through_integrator(ref["A"], ref["f32"]["a3"]), ref["C"]
    qa, da = sr.scalar_dofs(m)
    tag = f"bias {path} {cfg}"
    sr.compare(f"{tag} scalar dofs", got[:, da], C[:, da], twin[:, da], guard=INTEGRATOR_GUARD)
    ang = [k for adr, d, l in sr.free_joints(m) for k in range(d + 3, d + 6)]
    lin = [k for adr, d, l in sr.free_joints(m) for k in range(d, d + 3)]
    if ang:
        sr.compare(f"{tag} blocks, angular dofs", got[:, ang], C[:, ang], twin[:, ang])
        sr.compare(f"{tag} blocks, linear dofs", got[:, lin], C[:, lin], twin[:, lin])          # expected: zero (the frame sits at the centre of mass)
    sim.close()


def test_device_with_a_small_modelling_error_is_outside_the_bound(models, monkeypatch):
    """The comparisons above can fail: the device simulating cfg3 with ONE small modelling error (tests/test_smooth_ref.py: mutant - the hand's
    centre of mass 1 mm off, the forearm's iyy 1 % up, one damping coefficient 1 % up) is held to the reference of the unmutated model and
    must land outside the 8 x floor bound in the one-substep acceleration or in the velocity after fifty substeps, on at least 90 % of the
    states, for each mutation - the share the fp64 oracle of the same mutants reaches on the CPU."""
    from test_smooth_ref import MUTATIONS, mutant
    m = models["cfg3"]
    ref = sr.reference("cfg3", m, N, NSUB)
    vN = ref["f64"]["vN"]
    bound_a = sr.floor_of(ref["f32"]["a1"], ref["f64"]["a1"])[1]
    bound_v = sr.floor_of(sr.rel_vel(ref["f32"]["vN"], vN), sr.rel_vel(vN, vN))[1]
    for what in MUTATIONS:
        sim = hs.BatchSim(mutant(m, what), N)
        sim.set_state(np.zeros(N), ref["q"], ref["v"])
        a = (sim.step(ref["ctrl"], 1)[0][:, m.nq:].astype(np.float64) - ref["v"]) / m.timestep
        sim.set_state(np.zeros(N), ref["q"], ref["v"])
        v50 = sim.step(ref["ctrl"], NSUB)[0][:, m.nq:].astype(np.float64)
        ra, rv = sr.state_dist(a, ref["f64"]["a1"]) / bound_a, sr.state_dist(sr.rel_vel(v50, vN), sr.rel_vel(vN, vN)) / bound_v
        outside = (ra > 1) | (rv > 1)
        print(f"device, cfg3 with {what} (kernel_flags {sim.kernel_flags()}): outside the bound in {int(outside.sum())} of {N} states; "
              f"median distance {np.median(ra):.1f} x the bound in a, {np.median(rv):.1f} x in v after {NSUB} substeps")
        assert outside.mean() >= 0.9, what
        sim.close()


_FIFTY = {}


def fifty_substeps(models, path, cfg, monkeypatch):
    """obs after NSUB substeps from the reference states on one path; kept for the comparison of const with generic."""
    if (path, cfg) not in _FIFTY:
        m, sim = open_sim(models, path, cfg, monkeypatch)
        ref = sr.reference(cfg, m, N, NSUB)
        sim.set_debug(True)
        sim.set_state(np.zeros(N), ref["q"], ref["v"])
        obs, rew, done, ns = sim.step(ref["ctrl"], NSUB)
        assert (ns == NSUB).all() and not done.any() and not sim.bad_state()[1]
        assert_contact_free(sim, f"substep {NSUB}")
        sim.close()
        _FIFTY[(path, cfg)] = obs.astype(np.float64)
    return _FIFTY[(path, cfg)]


@pytest.mark.parametrize("path,cfg", PATHS)
def test_fifty_substeps_at_speed(models, path, cfg, monkeypatch):
    """(d) Fifty substeps on every path: |dv| / (1 + |v|) and |dq| against the fp64 oracle within their bounds (the fp32 build of the oracle
    leaves about 2e-6 .. 5e-6 and 6e-7)."""
    m = models[cfg]
    obs = fifty_substeps(models, path, cfg, monkeypatch)
    ref = sr.reference(cfg, m, N, NSUB)
    vN = ref["f64"]["vN"]
    tag = f"fifty {path} {cfg}"
    sr.compare(f"{tag} v/(1+|v|)", sr.rel_vel(obs[:, m.nq:], vN), sr.rel_vel(vN, vN), sr.rel_vel(ref["f32"]["vN"], vN))
    sr.compare(f"{tag} q", obs[:, :m.nq], ref["f64"]["qN"], ref["f32"]["qN"])


@pytest.mark.parametrize("cfg", ["cfg3", "cfg4"])
def test_const_and_generic_instances_agree_at_speed(models, cfg, monkeypatch):
    """(d) kin3.h against kin2.h on the same fast states after fifty substeps: both are fp32 results, each one floor away from fp64, so the
    bound is 8 x the fp32 oracle's distance from the fp64 oracle counted on both sides (16 x the one-sided floor)."""
    m = models[cfg]
    const, generic = fifty_substeps(models, "const", cfg, monkeypatch), fifty_substeps(models, "generic", cfg, monkeypatch)
    ref = sr.reference(cfg, m, N, NSUB)
    vN = ref["f64"]["vN"]
    tag = f"const vs generic {cfg}"
    sr.compare(f"{tag} v/(1+|v|)", sr.rel_vel(const[:, m.nq:], vN), sr.rel_vel(generic[:, m.nq:], vN), sr.rel_vel(ref["f32"]["vN"], vN), truth=sr.rel_vel(vN, vN))
    sr.compare(f"{tag} q", const[:, :m.nq], generic[:, :m.nq], ref["f32"]["qN"], truth=ref["f64"]["qN"])
