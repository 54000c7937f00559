"""On-policy rollouts on the device (include/hsrsim.h: hsr_batch_rollout_create .. hsr_rollout_planes_dev) against the numpy restatement of
tests/rollout_ref.py: GAE and the stored rows bit for bit, the statistics within the fp64 summation bound, the shuffle as the stated
permutation, calls out of order refused without a trace, shards with their own shuffle, and the Python surface fed from VecHSREnv.step.

Everything but the env-surface tests drives the C-ABI wrappers with synthetic device tensors from a seeded numpy generator, so that every branch
is reached by construction.  Main shape: cfg2 (obs_dim 17, nu 2: rows of 19 words padded to 20), 70 envs (two waves, the second partial),
a horizon of 5, minibatches of 96 (three full ones and one of 62)."""
import ctypes as C

import numpy as np
import pytest
import torch        # before the library: torch's HIP runtime must be the first one loaded into the process (as in test_gpu_episodes.py)

import rollout_ref as ref
from hsr_env_amd.env import GoalSpec, VecHSREnv
from hsr_env_amd.sim import RolloutSpec
from test_gpu_episodes import BLOCK_START, GEOFENCE, GOAL, SEED

pytestmark = pytest.mark.gpu
N, T, B, SUB = 70, 5, 96, 5
GAMMA, LAM = 0.99, 0.95
RSEED = 2 ** 35 + 4321              # the rollout's own seed
FIELDS = ("obs", "action", "logp", "value", "advantage", "ret", "index")
NAN_PAYLOAD = 0x7fc12345


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def magnitudes(rng, shape):
    """float32 with |x| in [1e-3, 1e3], either sign: no product of two of them is subnormal."""
    return (np.exp(rng.uniform(np.log(1e-3), np.log(1e3), shape)) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def make_inputs(seed, n, horizon, od=17, nu=2, planted=False):
    """What a rollout is fed: host arrays.  planted: envs with chosen reset kinds - all 0, all 1, cut at the last step, cut without a
    bootstrap call, cut then ended, a mixed second wave, a kind of 7 - and a NaN payload and -0 in the rows (needs n >= 70, horizon == 5)."""
    rng = np.random.default_rng(seed)
    x = dict(obs0=magnitudes(rng, (n, od)), next_obs=magnitudes(rng, (horizon, n, od)), act=magnitudes(rng, (horizon, n, nu)),
             logp=magnitudes(rng, (horizon, n)), value=magnitudes(rng, (horizon, n)), reward=magnitudes(rng, (horizon, n)),
             v_term=magnitudes(rng, (horizon, n)), last_value=magnitudes(rng, n),
             kind=rng.choice([0, 1, 2], (horizon, n), p=[0.7, 0.15, 0.15]).astype(np.uint8))
    x["skip_bootstrap"] = {1} if horizon > 1 else set()       # no bootstrap call after step 1: its truncated envs bootstrap from 0
    if planted:
        k = x["kind"]
        k[:, 0] = 0
        k[:, 1] = 1
        k[:, 2] = 0; k[horizon - 1, 2] = 2
        k[:, 3] = 0; k[1, 3] = 2
        k[:, 4] = 0; k[0, 4] = 2; k[1, 4] = 1
        k[:, 64:70] = np.array([[0, 1, 2, 0, 0, 2], [2, 0, 0, 1, 0, 0], [0, 0, 1, 2, 0, 1], [1, 2, 0, 0, 0, 0], [0, 0, 2, 1, 0, 2]], np.uint8)
        k[2, 10] = 7
        x["obs0"].view(np.uint32)[5, 3] = NAN_PAYLOAD
        x["next_obs"].view(np.uint32)[1, 65, 0] = 0x80000000
        x["next_obs"].view(np.uint32)[3, 69, 16] = NAN_PAYLOAD + 1
        x["act"].view(np.uint32)[2, 66, 1] = 0x80000000
    return x


class Rig:
    """One batch and the device copies of an input set; drive() feeds a device rollout and a restatement alike."""

    def __init__(self, sim, x):
        self.sim, self.x = sim, x
        self.d = {k: dev(v) for k, v in x.items() if isinstance(v, np.ndarray)}
        self.garbage = dev(np.full(sim.n, 777.0, np.float32))
        torch.cuda.synchronize()

    def make(self, horizon, offset=0, seed=RSEED, gamma=GAMMA, lam=LAM):
        od = self.x["obs0"].shape[1]
        ro = self.sim.rollout(RolloutSpec(seed=seed, env_offset=offset, horizon=horizon, obs_dim=od, gamma=gamma, lam=lam))
        return ro, ref.Store(self.sim.n, horizon, od, self.sim.nu, gamma, lam, seed=seed, env_offset=offset)

    def step(self, t, ro=None, store=None):
        d, x = self.d, self.x
        if ro is not None:
            ro.stage_dev(d["act"][t].data_ptr(), d["logp"][t].data_ptr(), d["value"][t].data_ptr())
            ro.close_dev(d["reward"][t].data_ptr(), d["kind"][t].data_ptr(), d["next_obs"][t].data_ptr())
            if t not in x["skip_bootstrap"]:
                ro.bootstrap_dev(self.garbage.data_ptr())          # the last call wins
                ro.bootstrap_dev(d["v_term"][t].data_ptr())
        if store is not None:
            store.stage(x["act"][t], x["logp"][t], x["value"][t])
            store.close(x["reward"][t], x["kind"][t], x["next_obs"][t])
            if t not in x["skip_bootstrap"]:
                store.bootstrap(np.full(self.sim.n, 777.0, np.float32))
                store.bootstrap(x["v_term"][t])

    def drive(self, ro=None, store=None):
        horizon = self.x["kind"].shape[0]
        if ro is not None:
            ro.begin_dev(self.d["obs0"].data_ptr())
        if store is not None:
            store.begin(self.x["obs0"])
        for t in range(horizon):
            self.step(t, ro, store)
        if ro is not None:
            ro.finish_dev(self.d["last_value"].data_ptr())
        if store is not None:
            store.finish(self.x["last_value"])

    def planes(self, ro, horizon):
        adv = torch.zeros((horizon, self.sim.n), dtype=torch.float32, device="cuda")
        ret = torch.zeros_like(adv)
        torch.cuda.synchronize()
        ro.planes_dev(adv.data_ptr(), ret.data_ptr())
        self.sim.sync()
        return adv.cpu().numpy(), ret.cpu().numpy()

    def minibatch(self, ro, epoch, first, count, normalize, rows=None, only=FIELDS):
        """The outputs as host arrays of `rows` rows (default count), filled with a sentinel before the call; `only`: the outputs passed."""
        rows = count if rows is None else rows
        od, nu = self.x["obs0"].shape[1], self.sim.nu
        shape = dict(obs=(rows, od), action=(rows, nu), logp=(rows,), value=(rows,), advantage=(rows,), ret=(rows,), index=(rows, 2))
        out = {k: torch.full(shape[k], -7, dtype=torch.int32 if k == "index" else torch.float32, device="cuda") for k in FIELDS}
        torch.cuda.synchronize()
        ro.minibatch_dev(epoch, first, count, normalize, *[out[k].data_ptr() if k in only else None for k in FIELDS])
        self.sim.sync()
        return {k: v.cpu().numpy() for k, v in out.items()}


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def stats_bound(value64, adv):
    """One float32 ulp of the fp64 value plus the fp64 summation bound M 2^-52 mean|adv|."""
    a = adv.astype(np.float64)
    return ulp32(value64) + a.size * 2.0 ** -52 * np.abs(a).mean()


@pytest.fixture(scope="module")
def run(models):
    """The main shape, driven once: three rollouts of one batch (env_offset 0, 70, 0) and their restatements, the first driven twice."""
    from hsr_env_amd.sim import BatchSim
    sim = BatchSim(models["cfg2"], N)
    rig = Rig(sim, make_inputs(1, N, T, planted=True))
    made = [rig.make(T, offset) for offset in (0, 70, 0)]
    for ro, store in made:
        rig.drive(ro, store)
    ro, store = made[0]
    first = dict(planes=rig.planes(ro, T), stats=ro.stats())
    rig.drive(ro)                                                       # begin from DONE, the same inputs once more
    second = dict(planes=rig.planes(ro, T), stats=ro.stats())
    yield dict(rig=rig, made=made, first=first, second=second)
    for ro, _ in made:
        ro.close()
    sim.close()


def test_gae_bit_for_bit(run):
    rig, (ro, store) = run["rig"], run["made"][0]
    x = rig.x
    assert ref.row_words(17, 2) == (19, 20)
    assert ro.state() == (ref.DONE, T) == (store.state, store.t)
    adv, ret = run["first"]["planes"]
    assert same(adv, store.adv) and same(ret, store.ret)
    k = x["kind"]
    assert (k == 7).any() and k[:, 0].max() == 0 and k[:, 1].min() == 1 and k[T - 1, 2] == 2 and k[1, 3] == 2 and (k[0, 4], k[1, 4]) == (2, 1)
    # the truncated step without a bootstrap call bootstrapped from 0, the one with a call from its value
    d1 = np.float32(np.float32(x["reward"][1, 3] + np.float32(0)) - x["value"][1, 3])
    assert adv[1, 3] == d1 and store.v_term[1, 3] == 0 and store.v_term[T - 1, 2] == x["v_term"][T - 1, 2] != 0
    # the rows as stored, through a whole epoch without normalisation
    out = rig.minibatch(ro, 0, 0, T * N, False)
    t, e = out["index"].T
    assert sorted(zip(t.tolist(), e.tolist())) == [(a, b) for a in range(T) for b in range(N)]
    acted_on = np.concatenate([x["obs0"][None], x["next_obs"][:-1]])                         # slot t + 1 holds the next_obs of close t
    assert same(out["obs"], acted_on[t, e]) and same(out["action"], x["act"][t, e])
    assert same(out["logp"], x["logp"][t, e]) and same(out["value"], x["value"][t, e])
    assert same(out["advantage"], store.adv[t, e]) and same(out["ret"], store.ret[t, e])
    got = out["obs"].view(np.uint32)
    assert got[(t == 0) & (e == 5), 3] == NAN_PAYLOAD and got[(t == 2) & (e == 65), 0] == 0x80000000 and got[(t == 4) & (e == 69), 16] == NAN_PAYLOAD + 1
    assert out["action"].view(np.uint32)[(t == 2) & (e == 66), 1] == 0x80000000


def test_statistics(run):
    store = run["made"][0][1]
    adv = run["first"]["planes"][0]
    want = ref.stats(adv)
    for name, got, w in zip(("mean", "std", "rstd"), run["first"]["stats"], want):
        bound = stats_bound(w, adv)
        print(f"{name}: device {got!r}, fp64 {w!r}, |difference| {abs(float(got) - w):.3e}, bound {bound:.3e}")
        assert abs(float(got) - w) <= bound, name
    assert same(np.array(run["first"]["stats"]), np.array([store.mean32, store.std32, store.rstd32]))
    # the same inputs once more: the same bits
    assert same(np.array(run["second"]["stats"]), np.array(run["first"]["stats"]))
    assert same(run["second"]["planes"][0], adv) and same(run["second"]["planes"][1], run["first"]["planes"][1])


def test_minibatches(run):
    rig, (ro, store) = run["rig"], run["made"][0]
    mean32, _, rstd32 = ro.stats()
    for epoch in (0, 1):
        for normalize in (True, False):
            seen = []
            for first in range(0, T * N, B):
                count = min(B, T * N - first)
                out = rig.minibatch(ro, epoch, first, count, normalize, rows=B)
                want = store.minibatch(epoch, first, count, normalize, mean32=mean32, rstd32=rstd32)
                for name in FIELDS:
                    assert same(out[name][:count], want[name]), (epoch, normalize, first, name)
                    assert np.all(out[name][count:] == -7), (epoch, first, name)              # nothing is written past `count`
                seen += list(map(tuple, out["index"][:count].tolist()))
            assert [first for first in range(0, T * N, B)] == [0, 96, 192, 288] and count == 62
            assert sorted(seen) == [(t, e) for t in range(T) for e in range(N)]                # each of the 350 exactly once
    a, b = (rig.minibatch(ro, epoch, 0, T * N, True)["index"] for epoch in (0, 1))
    assert (a != b).any(1).sum() > T * N // 2                                                  # another epoch, another order
    # normalised advantages are mul(sub(adv, mean32), rstd32) with the device's own mean32 / rstd32
    out = rig.minibatch(ro, 0, 0, T * N, True)
    t, e = out["index"].T
    assert same(out["advantage"], ref.normalized(store.adv[t, e], mean32, rstd32))
    # NULL outputs are skipped
    some = rig.minibatch(ro, 0, 96, 96, True, only=("advantage", "index"))
    full = rig.minibatch(ro, 0, 96, 96, True)
    for name in FIELDS:
        assert same(some[name], full[name]) if name in ("advantage", "index") else np.all(some[name] == -7), name
    rig.minibatch(ro, 0, 0, 5, False, only=())


@pytest.mark.parametrize("n,horizon", [(64, 4), (1, 1)])
def test_edge_shapes(models, n, horizon):
    """64 x 4: M = 256 is the shuffle's whole domain (h = 4), no walk; 1 x 1: M = 1 in a domain of 4."""
    from hsr_env_amd.sim import BatchSim
    sim = BatchSim(models["cfg2"], n)
    rig = Rig(sim, make_inputs(2, n, horizon))
    ro, store = rig.make(horizon, gamma=1.0, lam=0.5)
    rig.drive(ro, store)
    adv, ret = rig.planes(ro, horizon)
    assert same(adv, store.adv) and same(ret, store.ret)
    got = ro.stats()
    for g, w in zip(got, ref.stats(adv)):
        assert abs(float(g) - w) <= stats_bound(w, adv)
    M = n * horizon
    assert ref.half_bits(M) == (4 if M == 256 else 1)
    seen = []
    for first in range(0, M, 50):
        count = min(50, M - first)
        out = rig.minibatch(ro, 3, first, count, True, rows=50)
        want = store.minibatch(3, first, count, True, mean32=got[0], rstd32=got[2])
        for name in FIELDS:
            assert same(out[name][:count], want[name]) and np.all(out[name][count:] == -7), (first, name)
        seen += list(map(tuple, out["index"][:count].tolist()))
    assert sorted(seen) == [(t, e) for t in range(horizon) for e in range(n)]
    ro.next()
    assert ro.state() == (ref.READY, 0)
    ro.close()
    sim.close()


def test_refusals(models):
    from hsr_env_amd.sim import BatchSim
    sim = BatchSim(models["cfg2"], 9)
    L = sim._L
    # ---- create
    ok = dict(seed=1, env_offset=0, horizon=3, obs_dim=17, gamma=GAMMA, lam=LAM)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(horizon=0), dict(horizon=-2), dict(obs_dim=0), dict(obs_dim=-1), dict(obs_dim=2 ** 20 + 1), dict(gamma=-0.01), dict(gamma=1.01),
                dict(gamma=nan), dict(gamma=inf), dict(lam=-0.01), dict(lam=1.01), dict(lam=nan), dict(lam=-inf),
                dict(horizon=2 ** 31 - 1), dict(horizon=(2 ** 31 + 8) // 9),        # T N >= 2^31
                dict(horizon=2 ** 20, obs_dim=2 ** 20)):                             # 2^43 bytes of rows
        with pytest.raises(AssertionError):
            sim.rollout(RolloutSpec(**{**ok, **bad}))
    handle = C.c_void_p()
    assert L.hsr_batch_rollout_create(sim._b, None, C.byref(handle)) == -1 and L.hsr_batch_rollout_create(sim._b, C.byref(RolloutSpec(**ok)), None) == -1
    assert L.hsr_batch_rollout_create(None, C.byref(RolloutSpec(**ok)), C.byref(handle)) == -1 and not handle.value
    # ---- protocol: in every state every call the state does not allow is refused and the books stay
    rig = Rig(sim, make_inputs(3, 9, 3))
    ro, store = rig.make(3, seed=1)
    d = rig.d
    stage = lambda: ro.stage_dev(d["act"][0].data_ptr(), d["logp"][0].data_ptr(), d["value"][0].data_ptr())
    close = lambda: ro.close_dev(d["reward"][0].data_ptr(), d["kind"][0].data_ptr(), d["next_obs"][0].data_ptr())
    boot = lambda: ro.bootstrap_dev(rig.garbage.data_ptr())
    finish = lambda: ro.finish_dev(rig.garbage.data_ptr())
    mini = lambda: ro.minibatch_dev(0, 0, 1, 0)
    planes = lambda: ro.planes_dev(None, None)

    def refused(*calls):
        before = ro.state()
        for call in calls:
            with pytest.raises(AssertionError):
                call()
        assert ro.state() == before

    assert ro.state() == (ref.EMPTY, 0)
    refused(stage, close, boot, finish, ro.next, ro.stats, mini, planes)
    ro.begin_dev(d["obs0"].data_ptr()); store.begin(rig.x["obs0"])
    refused(close, boot, finish, ro.next, ro.stats, mini, planes)       # READY(0)
    for t in range(3):
        ro.stage_dev(d["act"][t].data_ptr(), d["logp"][t].data_ptr(), d["value"][t].data_ptr())
        assert ro.state() == (ref.STAGED, t)
        refused(stage, boot, finish, ro.next, ro.stats, mini, planes)
        refused(lambda: ro.close_dev(None, d["kind"][0].data_ptr(), d["next_obs"][0].data_ptr()))
        ro.close_dev(d["reward"][t].data_ptr(), d["kind"][t].data_ptr(), d["next_obs"][t].data_ptr())
        if t != 1:
            ro.bootstrap_dev(d["v_term"][t].data_ptr())
        refused(close, ro.next, ro.stats, mini, planes, *([finish] if t < 2 else [stage]))
    for t in range(3):
        rig.step(t, None, store)
    ro.finish_dev(d["last_value"].data_ptr()); store.finish(rig.x["last_value"])
    assert ro.state() == (ref.DONE, 3)
    base_planes, base_rows, base_stats = rig.planes(ro, 3), rig.minibatch(ro, 0, 0, 27, True), ro.stats()
    refused(stage, close, boot, finish)
    for first, count in ((0, 0), (0, -1), (-1, 2), (27, 1), (0, 28), (26, 2), (2 ** 31 - 1, 2 ** 31 - 1)):
        refused(lambda: ro.minibatch_dev(0, first, count, 0))
    # the refused calls left no trace: the same bytes as before them, and the store is the one the valid calls alone built
    after_planes, after_rows = rig.planes(ro, 3), rig.minibatch(ro, 0, 0, 27, True)
    assert same(after_planes[0], base_planes[0]) and same(after_planes[1], base_planes[1]) and same(np.array(ro.stats()), np.array(base_stats))
    assert same(after_planes[0], store.adv) and same(after_planes[1], store.ret)
    want = store.minibatch(0, 0, 27, True, mean32=base_stats[0], rstd32=base_stats[2])
    for name in FIELDS:
        assert same(after_rows[name], base_rows[name]) and same(after_rows[name], want[name]), name
    ro.next()
    refused(close, boot, finish, ro.next, ro.stats, mini, planes)
    # ---- the batch goes first: the handle refuses everything but its own destruction
    sim.close()
    for call in (ro.state, stage, close, boot, finish, ro.next, ro.stats, mini, planes, lambda: ro.begin_dev(d["obs0"].data_ptr())):
        with pytest.raises(AssertionError, match="destroyed"):
            call()
    ro.close()
    ro.close()


def test_a_shard_draws_its_own_shuffle(run):
    rig = run["rig"]
    (at0, _), (at70, store70), (at0_again, _) = run["made"]
    a, b, c = (rig.minibatch(ro, 2, 0, T * N, False) for ro in (at0, at70, at0_again))
    assert not same(a["index"], b["index"])
    want = store70.minibatch(2, 0, T * N, False)
    for name in FIELDS:
        assert same(a[name], c[name]), name
        assert same(b[name], want[name]), name


def test_env_surface(models):
    m = models["cfg2"]
    kw = dict(model=m, goals=[GoalSpec("block0", GOAL, GEOFENCE)], starts={"block0joint": BLOCK_START}, steps_per_action=SUB, n_envs=N)
    w = dev(np.random.default_rng(9).uniform(-1, 1, m.nq + m.nv).astype(np.float32))

    def loop(with_rollout, with_replay=False, rollouts=2):
        env = VecHSREnv(auto_reset=True, max_episode_steps=3, **kw)
        env.seed(SEED)
        ro = env.make_rollout(T) if with_rollout else None
        replay = env.make_replay(7) if with_replay else None
        obs = env.reset()
        results, checked = [], []
        for _ in range(rollouts):
            hist = dict(value=[], reward=[], kind=[], v_term=[], obs=[obs.copy()])
            for t in range(T):
                a = env.sample_action_dev()
                env.sim.sync()                                          # the draw ran on the batch's stream
                if ro is not None:
                    assert same(ro.obs.cpu().numpy(), obs)              # what the policy acts on is what the env returned
                    value, logp = ro.obs @ w, -(a * a).sum(1)
                    ro.stage(a, logp, value)
                    hist["value"].append(value.cpu().numpy())
                obs, rew, done, info = env.step(a)
                results.append((obs.copy(), rew.copy(), done.copy(), info["terminal_observation"].copy()))
                if ro is not None:
                    assert same(ro.terminal_obs.cpu().numpy(), info["terminal_observation"])
                    v_term = ro.terminal_obs @ w
                    ro.bootstrap(v_term)
                    hist["v_term"].append(v_term.cpu().numpy())
                    hist["reward"].append(rew.copy())
                    hist["kind"].append(np.where(info["TimeLimit.truncated"], 2, np.where(done, 1, 0)).astype(np.uint8))
                    hist["obs"].append(obs.copy())
            if ro is None:
                continue
            last = ro.obs @ w
            ro.finish(last)
            adv, ret = ro.advantages().cpu().numpy(), ro.returns().cpu().numpy()
            kind = np.stack(hist["kind"])
            want_adv, want_ret = ref.gae(np.stack(hist["reward"]), np.stack(hist["value"]), kind, np.stack(hist["v_term"]), last.cpu().numpy(), 0.99, 0.95)
            # the advantages of the host's own history: the stored reward and kind are what step() returned
            assert same(adv, want_adv) and same(ret, want_ret)
            mean, std, rstd = ro.stats()
            seen = []
            for mb in ro.minibatches(B, epoch=1):
                host = {k: v.cpu().numpy() for k, v in mb.items()}
                t, e = host["index"].T
                assert same(host["obs"], np.stack(hist["obs"])[t, e]) and same(host["value"], np.stack(hist["value"])[t, e])
                assert same(host["advantage"], ref.normalized(want_adv[t, e], mean, rstd)) and same(host["ret"], want_ret[t, e])
                seen += list(zip(t.tolist(), e.tolist()))
            assert sorted(seen) == [(t, e) for t in range(T) for e in range(N)]
            checked.append((kind, adv))
            ro.next()
            assert ro.state() == (ref.READY, 0)
        return env, ro, replay, results, checked

    env, ro, _, results, checked = loop(True)
    kinds = np.concatenate([k for k, _ in checked])
    assert (kinds == 0).any() and (kinds == 1).any() and (kinds == 2).any()                    # goes on, done, cut by the time limit
    # a step without a staged action is refused before anything runs
    with pytest.raises(ValueError, match="stage"):
        env.step(env.sample_action_dev())
    # fork restarts the rollout from the current rows
    a = env.sample_action_dev()
    env.sim.sync()
    ro.stage(a, -(a * a).sum(1), ro.obs @ w)
    env.step(a)
    assert ro.state() == (ref.READY, 1)
    env.fork(0, 1)
    assert ro.state() == (ref.READY, 0) and same(ro.obs.cpu().numpy(), env._last_obs.astype(np.float32))
    assert np.array_equal(env._last_obs[0], env._last_obs[1])
    env.close()
    # the rollout changes no result: a twin of the same seed without one
    plain, none, _, plain_results, _ = loop(False)
    assert none is None
    for (o, r, d, t), (o2, r2, d2, t2) in zip(results, plain_results):
        assert same(o, o2) and same(r, r2) and np.array_equal(d, d2) and same(t, t2)
    plain.close()
    # it coexists with a replay: the same results and advantages, and the ring holds the steps
    both, _, replay, both_results, both_checked = loop(True, with_replay=True)
    assert replay.state() == (7, 10 % 7, 10)
    for (o, r, d, t), (o2, r2, d2, t2) in zip(results, both_results):
        assert same(o, o2) and same(r, r2) and np.array_equal(d, d2) and same(t, t2)
    for (k, adv), (k2, adv2) in zip(checked, both_checked):
        assert np.array_equal(k, k2) and same(adv, adv2)
    both.close()
    with pytest.raises(ValueError, match="auto_reset"):
        VecHSREnv(**kw).make_rollout(T)


@pytest.mark.parametrize("with_replay", [False, True])
def test_env_surface_with_the_openai_observation(models, with_replay):
    """Rows are the 25-float observation: the policy rows and the terminal rows are two device buffers of the loop, which an attached
    replay reads too."""
    m = models["cfg3"]
    env = VecHSREnv(model=m, goals=[GoalSpec("block0", GOAL, GEOFENCE)], starts={"block0joint": BLOCK_START}, steps_per_action=SUB, n_envs=5,
                    obs_type="openai", auto_reset=True, max_episode_steps=2)
    ro = env.make_rollout(3)
    replay = env.make_replay(4, her_ratio=0.0) if with_replay else None
    obs = env.reset()
    w = dev(np.random.default_rng(4).uniform(-1, 1, 25).astype(np.float32))
    acted_on, terminal, values = [], [], []
    for _ in range(3):
        assert tuple(ro.obs.shape) == (5, 25) and same(ro.obs.cpu().numpy(), obs)
        a = env.sample_action_dev()
        env.sim.sync()
        value = ro.obs @ w
        ro.stage(a, -(a * a).sum(1), value)
        acted_on.append(obs.copy()); values.append(value.cpu().numpy())
        obs, _, _, info = env.step(a)
        assert same(ro.terminal_obs.cpu().numpy(), info["terminal_observation"])
        terminal.append(info["terminal_observation"].copy())
        ro.bootstrap(ro.terminal_obs @ w)
    ro.finish(ro.obs @ w)
    for mb in ro.minibatches(15, epoch=0, normalize=False):
        host = {k: v.cpu().numpy() for k, v in mb.items()}
        t, e = host["index"].T
        assert same(host["obs"], np.stack(acted_on)[t, e]) and same(host["value"], np.stack(values)[t, e])
    if replay is not None:
        out = {k: v.cpu().numpy() for k, v in replay.sample(32).items()}
        e, slot = out["index"][:, 0], out["index"][:, 1]
        assert same(out["obs"], np.stack([acted_on[s][i] for s, i in zip(slot, e)]))
        assert same(out["next_obs"], np.stack([terminal[s][i] for s, i in zip(slot, e)]))
    env.close()
