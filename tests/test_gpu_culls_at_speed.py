"""The narrowphase item list and the separation margins of the persistent kernel (csrc/persist.h) with a FAST arm and a thrown block: the list is built from
culls that ask "closer than HSR_SKIN" and kept until 2 acc_move >= skin, acc_move summing the per-substep bound 1.25 h (|v_geom| + |w| rbound) + 1e-7; the
margins of the convex pairs are eaten up by the same bounds.  The existing checks move the arm at 0.05 rad/s or not at all (static1), so the |w| rbound term
of a link's bound is never exercised at speed.  Here every env's fastest geom moves 0.2 .. 5 mm per substep (the list lives 1 .. 25 substeps) and the block
flies at the hand at 0.2 .. 2 m/s, spinning at up to 20 rad/s (a quarter of the envs: spinning in place next to the hand, see fast_states).  Launches of 1, 2, 3, 5, 8, 13 and 21 substeps from the same start state are held to
  * the same launch culling every substep (test hook 64): state, warm start, contact counts and contacts bit for bit,
  * the chain kernels at the state the reported contacts belong to (cull and narrowphase from scratch): no contact of depth >= 2e-6 is missing,
  * exact geometry (tests/geom_checks.py, fp64 kinematics of hsr_env_amd/model.py): a block pair that overlaps by >= 2e-6 has a contact,
and the case must have teeth: pairs that were provably farther apart than the skin at launch start and touch at its end - each one went through a rebuild.
One fixture per configuration does all device work once; the tests read what it left."""
import numpy as np
import pytest

import cull_ref
import geom_checks as gc
from hsr_env_amd import model as hm
from hsr_env_amd import sim as hs
from oracle.oracle import OracleSim
from test_gpu_parity import random_states

pytestmark = pytest.mark.gpu

N = 256
LAUNCHES = (1, 2, 3, 5, 8, 13, 21)
MOVE_LO, MOVE_HI = 0.2e-3, 5e-3          # metres per substep of the fastest geom
DEMAND = 2e-6
SEED = {"cfg3": 31, "cupboard": 32}


def kin(m, q):
    """fp64 link poses and dof axes of one env"""
    xpos, xquat = hm.link_kinematics(m, q)
    return xpos, xquat, hm.dof_motion(m, xpos, xquat, q)


def geom_moves(m, q, v):
    """per geom: h (|v_geom| + |w| rbound), the kernel's measure of how far the geom can move in one substep, in fp64"""
    xpos, xquat, (ang, lin, anchor) = kin(m, q)
    out = np.zeros(m.ngeom)
    for g in range(m.ngeom):
        l = int(m.geom_link[g])
        if l == 0:
            continue
        jp, jr = hm.point_jacobian(m, ang, lin, anchor, l, xpos[l] + hm.quat_to_mat(xquat[l]) @ m.geom_pos[g])
        out[g] = m.timestep * (np.linalg.norm(jp @ v) + np.linalg.norm(jr @ v) * m.geom_rbound[g])
    return out


def block_geom(m):
    return int(np.flatnonzero(m.geom_link == int(m.body_link[m.body_id(m.block_body())]))[0])


def fast_states(m, n, rng):
    """random_states with the robot's joint velocities scaled so that the fastest robot geom of env e moves target[e] per substep (log-uniform over
    MOVE_LO .. MOVE_HI) and the block put 3 .. 10 cm from the point between the finger tips, free of contact, flying at that point.  The targets ascend
    with the env index: the envs of a wave share one list (one env's move rebuilds it for all), so a slow arm keeps its long-lived list only next to slow
    arms.  Every second env of the slower half is a SPINNER: its block hardly translates (< 0.05 m/s) and spins at 10 .. 20 rad/s, so that its corners
    sweep 1 .. 2 mm per substep while its origin stands still - the |w| rbound term of the move bound is then all that accounts for it, under a list
    that lives 10 to 20 substeps (with that term dropped from persist.h this module fails; with thrown blocks alone it passed)"""
    q, v, ctrl = random_states(m, n, rng)
    qa, da = m.scalar_joints()
    a = int(m.free_joint_qadrs()[0])
    gb = block_geom(m)
    lb = int(m.geom_link[gb]); d0 = int(m.link_dofadr[lb])
    ll, lr = int(m.body_link[m.body_id("hand_l_distal_link")]), int(m.body_link[m.body_id("hand_r_distal_link")])
    target = np.sort(np.exp(rng.uniform(np.log(MOVE_LO), np.log(MOVE_HI), n)))
    robot = np.array([g for g in range(m.ngeom) if int(m.geom_link[g]) not in (0, lb)])
    o = OracleSim(m)
    for e in range(n):
        v[e] = 0
        vd = np.zeros(m.nv); vd[da] = rng.normal(size=len(da))
        v[e] = vd * target[e] / geom_moves(m, q[e], vd)[robot].max()
        xpos, _, _ = kin(m, q[e])
        hand = 0.5 * (xpos[ll] + xpos[lr])
        for attempt in range(200):
            u = rng.normal(size=3); u /= np.linalg.norm(u)
            q[e, a:a + 3] = hand + u * rng.uniform(0.03, 0.07 if e < n // 2 and e % 2 == 1 else 0.10)
            q[e, a + 3:a + 7] = gc.random_quat(rng)
            o.qpos[:] = q[e]; o.qvel[:] = 0; o.forward()
            c = o.contacts()
            if not len(c) or not np.any((c[:, 13] == gb) | (c[:, 14] == gb)):
                break
        else:
            raise AssertionError("no contact-free place for the block")
        spinner = e < n // 2 and e % 2 == 1
        v[e, d0:d0 + 3] = -u * (rng.uniform(0, 0.05) if spinner else np.exp(rng.uniform(np.log(0.2), np.log(2.0))))
        w = rng.normal(size=3)
        v[e, d0 + 3:d0 + 6] = w / np.linalg.norm(w) * (rng.uniform(10, 20) if spinner else rng.uniform(0, 20))
    return q, v, ctrl, target


def launch(m, q, v, ctrl, k, hook):
    """a fresh batch (no warm start, no margins, no list) stepped k substeps -> dict of everything the comparisons read"""
    sim = hs.BatchSim(m, len(q))
    assert sim.is_persistent()
    sim.set_debug(1 | hook)
    sim.set_state(np.zeros(len(q)), q, v)
    sim.step(ctrl, k)
    t, qq, vv = sim.get_state()
    out = dict(q=qq, v=vv, t=t, warm=sim.get_warmstart(), ncon=sim.get_field(hs.F_NCON), con=sim.get_field(hs.F_CONTACT))
    assert not sim.bad_state()[1]
    sim.close()
    return out


def pair_depths(m, con):
    """[n, npair]: the deepest contact of every pair (0: none)"""
    d = np.zeros((con.shape[0], m.npair))
    for p in range(m.npair):
        rows = con[:, int(m.pair_slot[p]):int(m.pair_slot[p + 1]), 6]
        d[:, p] = np.maximum(-np.where(rows <= 0, rows, 0.0).min(1), 0.0) if rows.shape[1] else 0.0
    return d


def pair_has(m, con):
    h = np.zeros((con.shape[0], m.npair), bool)
    for p in range(m.npair):
        h[:, p] = (con[:, int(m.pair_slot[p]):int(m.pair_slot[p + 1]), 6] <= 0).any(1)
    return h


def exact_pair(m, q, g1, g2):
    """exact_penetration of two geoms at the fp64 kinematics of state q (a cylinder: the inscribed 720-gon prism, radius short by 1e-5 r)"""
    xpos, xquat, _ = kin(m, q.astype(np.float64))
    xmat = np.array([hm.quat_to_mat(x) for x in xquat])
    va = gc.shape_vertices(m, g1, *gc.geom_pose(m, xpos, xmat, g1))
    vb = gc.shape_vertices(m, g2, *gc.geom_pose(m, xpos, xmat, g2))
    return gc.exact_penetration(va, vb)[0]


def sphere_gap(m, q, pairs):
    """distance of the bounding spheres of the given pairs (negative: they overlap) - the cheap filter in front of exact_pair"""
    xpos, xquat, _ = kin(m, q.astype(np.float64))
    c = np.array([xpos[int(m.geom_link[g])] + hm.quat_to_mat(xquat[int(m.geom_link[g])]) @ m.geom_pos[g] for g in range(m.ngeom)])
    return np.array([np.linalg.norm(c[g1] - c[g2]) - m.geom_rbound[g1] - m.geom_rbound[g2] for g1, g2 in pairs])


@pytest.fixture(scope="module", params=["cfg3", "cupboard"])
def runs(request, models):
    cfg = request.param
    m = models[cfg]
    rng = np.random.default_rng(SEED[cfg])
    q, v, ctrl, target = fast_states(m, N, rng)
    q32, v32 = q.astype(np.float32), v.astype(np.float32)
    kept, every = {}, {}
    for k in sorted(set(LAUNCHES) | {k - 1 for k in LAUNCHES if k > 1}):
        kept[k] = launch(m, q32, v32, ctrl, k, 0)
        if k in LAUNCHES:
            every[k] = launch(m, q32, v32, ctrl, k, 64)
    chain = {}
    ref = hs.BatchSim(m, N)
    ref.set_persistent(False)
    for k in LAUNCHES:
        qs, vs = (q32, v32) if k == 1 else (kept[k - 1]["q"], kept[k - 1]["v"])
        ref.set_state(np.zeros(N), qs, vs)
        ref.forward()
        chain[k] = dict(q=qs, con=ref.get_field(hs.F_CONTACT))
    ref.close()
    return dict(cfg=cfg, m=m, q=q, v=v, target=target, kept=kept, every=every, chain=chain)


def test_the_speed_range_is_populated(runs):
    """the fastest robot geom of every env moves 0.2 .. 5 mm per substep by the kernel's own measure, evaluated on the host in fp64, and every fifth of the
    range (log scale) holds envs: with HSR_SKIN = 1 cm the list lives between 1 and about 25 substeps"""
    m, q, v = runs["m"], runs["q"], runs["v"]
    gb = block_geom(m)
    robot = [g for g in range(m.ngeom) if int(m.geom_link[g]) not in (0, int(m.geom_link[gb]))]
    mv = np.array([geom_moves(m, q[e], v[e])[robot].max() for e in range(N)])
    assert np.allclose(mv, runs["target"], rtol=1e-9)
    assert mv.min() >= MOVE_LO and mv.max() <= MOVE_HI
    hist = np.histogram(np.log(mv), bins=np.linspace(np.log(MOVE_LO), np.log(MOVE_HI), 6))[0]
    life = cull_ref.SKIN / (2 * 1.25 * mv)
    print(f"{runs['cfg']}: fastest geom {mv.min() * 1e3:.3f} .. {mv.max() * 1e3:.3f} mm per substep, envs per fifth of the range {hist.tolist()}; list life {life.min():.1f} .. {life.max():.1f} substeps")
    assert hist.min() >= N // 20, hist
    assert life.min() < 1.0 and life.max() > 15.0


@pytest.mark.parametrize("k", LAUNCHES)
def test_kept_list_equals_culling_every_substep(runs, k):
    a, b = runs["kept"][k], runs["every"][k]
    assert np.isfinite(a["q"]).all() and np.isfinite(a["v"]).all(), "the case must stay finite"
    for f in ("q", "v", "t", "warm", "ncon", "con"):
        diff = np.flatnonzero((a[f] != b[f]).reshape(N, -1).any(1))
        assert diff.size == 0, f"{runs['cfg']}, {k} substeps: {f} differs in envs {diff[:8].tolist()} between the kept list and culling every substep"


def test_no_contact_of_the_chain_is_missing(runs):
    """the contacts a launch of k substeps reports belong to the state after k - 1 substeps; the chain kernels cull and collide that state from scratch.
    No pair may have a chain contact of depth >= 2e-6 where the persistent launch has none; shallower differences are counted"""
    m = runs["m"]
    tot = miss_shallow = extra = 0
    for k in LAUNCHES:
        hp, hc = pair_has(m, runs["kept"][k]["con"]), pair_has(m, runs["chain"][k]["con"])
        dc = pair_depths(m, runs["chain"][k]["con"])
        missing = hc & ~hp
        deep = np.argwhere(missing & (dc >= DEMAND))
        assert deep.size == 0, (f"{runs['cfg']}, {k} substeps: (env, pair) {deep[:6].tolist()} have a chain contact of depth "
                                f"{[float(dc[e, p]) for e, p in deep[:6]]} and none from the persistent kernel")
        tot += int(hc.sum()); miss_shallow += int(missing.sum()); extra += int((hp & ~hc).sum())
    print(f"{runs['cfg']}: {tot} (env, pair) contacts of the chain over {len(LAUNCHES)} launches; missing below 2e-6: {miss_shallow}, persistent only: {extra}")
    assert tot > 50 * len(LAUNCHES)


def block_pairs(m, convex_only):
    gb = block_geom(m)
    return [(p, int(m.pair_geom1[p]), int(m.pair_geom2[p])) for p in range(m.npair)
            if gb in (int(m.pair_geom1[p]), int(m.pair_geom2[p])) and int(m.geom_type[int(m.pair_geom1[p])]) != hm.GEOM_PLANE
            and (not convex_only or int(m.pair_fn[p]) == hm.FN_CONVEX)]


def test_overlapping_block_pairs_have_a_contact(runs):
    """at most 300 (env, launch) samples where the block's bounding sphere is within 3 cm of a hull's or the wrist cylinder's: every convex pair of the
    block whose exact penetration depth is >= 2e-6 there has a contact in its slots"""
    m = runs["m"]
    pairs = block_pairs(m, True)
    cand = []
    for k in LAUNCHES:
        qs = runs["chain"][k]["q"]
        for e in range(N):
            gap = sphere_gap(m, qs[e], [(g1, g2) for _, g1, g2 in pairs])
            if gap.min() < 0.03:
                cand.append((float(gap.min()), k, e, gap))
    cand.sort(key=lambda c: c[0])
    n_pen = n_pairs = 0
    for _, k, e, gap in cand[:300]:
        has = pair_has(m, runs["kept"][k]["con"][e:e + 1])[0]
        for (p, g1, g2), sg in zip(pairs, gap):
            if sg >= 0:
                continue
            n_pairs += 1
            de = exact_pair(m, runs["chain"][k]["q"][e], g1, g2)
            if de >= DEMAND:
                n_pen += 1
                assert has[p], f"{runs['cfg']}, {k} substeps, env {e}: geoms {g1} and {g2} overlap by {de:.3e} and have no contact"
    print(f"{runs['cfg']}: {min(len(cand), 300)} of {len(cand)} samples, {n_pairs} pairs with overlapping spheres, {n_pen} overlapping by >= 2e-6: all have a contact")
    assert n_pen >= 30


def test_contacts_appear_on_pairs_that_started_off_the_list(runs):
    """teeth: (env, pair) cases with a contact at the end of a launch whose shapes were provably farther apart than HSR_SKIN at its start (-depth of
    exact_penetration is a lower bound of the distance; 1e-6 on top covers the prism inside the cylinder) - the pair was not on the first list, so only a
    rebuild at the right time can have produced the contact.  Fewer than 20 such cases and the case has not exercised a rebuild"""
    m = runs["m"]
    pairs = block_pairs(m, False)
    seen, far = set(), {}
    for k in LAUNCHES:
        has = pair_has(m, runs["kept"][k]["con"])
        for p, g1, g2 in pairs:
            for e in np.flatnonzero(has[:, p]):
                key = (int(e), p)
                if key not in far:
                    far[key] = -exact_pair(m, runs["q"][e].astype(np.float32), g1, g2) > cull_ref.SKIN + 1e-6
                if far[key]:
                    seen.add(key)
    print(f"{runs['cfg']}: {len(seen)} (env, pair) cases off the list at launch start and in contact at a launch's end, of {len(far)} with a contact")
    assert len(seen) >= 20
