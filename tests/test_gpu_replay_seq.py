"""The device replay's window sampler (include/hsrsim.h: hsr_replay_sample_seq_dev) against the numpy restatement of
tests/replay_seq_ref.py: windows are the stated rows bit for bit and zero past their length, reward, done and the n-step outputs are the
stated function for every sample whose distances are clear of the geofence, seq_len = 1 is hsr_replay_sample_dev, the same (seed, draw)
gives the same bytes, every output may be NULL, nothing is written past the batch, refused calls leave no trace, and the Python surface
returns the ring's rows.

Main shape: the one of test_gpu_replay.py (cfg2, 70 envs, 5 substeps, a ring of 7 that wraps, episodes of at most 3 steps, 12 env-steps,
minibatches of 193) with seq_len 1, 2, 3, 5 (longer than any episode: always padding) and 7 (the capacity), her_ratio 0, 0.5, 1, gamma 0.9.
Second shape: episodes of at most 6 steps, a ring of 16, 20 env-steps, seq_len 4, minibatches of 4096: windows cut by seq_len.  In the
main shape the block rests where its episode put it (it moves about a micrometre per env-step), so a relabelled goal is reached by every
step of its episode and nstep is 1 whenever her_ratio is 1.  The second shape therefore moves the block between env-steps (a host
set_state to a random place on the table): achieved goals then differ by centimetres inside an episode, and relabelled windows miss,
reach in the middle and reach at their end."""
import numpy as np
import pytest
import torch        # before the library: torch's HIP runtime must be the first one loaded into the process (as in test_gpu_episodes.py)

import replay_seq_ref as seq
from hsr_env_amd.env import GoalSpec, VecHSREnv
from hsr_env_amd.sim import ReplaySeqOut
from test_gpu_episodes import BLOCK_START, GEOFENCE, GOAL, MOCAP_BODY, cfg2_spec
from test_gpu_replay import FIELDS, LIMIT, SUB, B, Loop, N, STEPS, T, same

pytestmark = pytest.mark.gpu
GAMMA = 0.9
LENS, HERS = (1, 2, 3, 5, 7), (0.0, 0.5, 1.0)
T2, LIMIT2, STEPS2, L2, B2 = 16, 6, 20, 4, 4096
COPIED = ("obs", "action", "next_obs", "achieved_next", "goal", "length", "index")
DERIVED = ("reward", "done", "nstep", "nstep_return", "nstep_discount", "nstep_obs", "nstep_done")
SENTINEL = 0xA5


def shapes(batch, L, od, nu):
    f32, u8, i32 = torch.float32, torch.uint8, torch.int32
    return dict(obs=((batch, L, od), f32), action=((batch, L, nu), f32), next_obs=((batch, L, od), f32), achieved_next=((batch, L, 3), f32),
                goal=((batch, 3), f32), reward=((batch, L), f32), done=((batch, L), u8), length=((batch,), i32), nstep=((batch,), i32),
                nstep_return=((batch,), f32), nstep_discount=((batch,), f32), nstep_obs=((batch, od), f32), nstep_done=((batch,), u8),
                index=((batch, 4), i32))


def sentinel_tensors(batch, L, od, nu):
    """Every output one row longer than the batch, every byte SENTINEL."""
    dev = torch.device("cuda", 0)
    out = {}
    for name, (shape, dtype) in shapes(batch + 1, L, od, nu).items():
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        out[name] = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device=dev).view(dtype).view(shape)
    torch.cuda.synchronize()
    return out


def untouched(t):
    return bool((t.contiguous().view(torch.uint8) == SENTINEL).all().item())


def struct_of(tensors, skip=()):
    return ReplaySeqOut(**{"act" if k == "action" else k: None if k in skip else v.data_ptr() for k, v in tensors.items()})


def sample_seq(loop, which, draw, batch, L, her, gamma=GAMMA, skip=()):
    """Windows `draw` of replay `which` as host arrays (the first `batch` rows); the row past the batch and every skipped output must
    still hold the sentinel."""
    t = sentinel_tensors(batch, L, loop.od, loop.sim.nu)
    loop.reps[which].sample_seq_dev(draw, batch, L, her, gamma, struct_of(t, skip))
    loop.sim.sync()
    for name, v in t.items():
        assert untouched(v[batch:]), f"{name}: written past row batch - 1"
        if name in skip:
            assert untouched(v), f"{name}: written though its pointer was NULL"
    return {k: v[:batch].cpu().numpy() for k, v in t.items() if k not in skip}


def clear_samples(out):
    """A sample is clear when no step distance of its window, |achieved_next - goal| in fp64, lies within 1e-6 of the geofence (inside
    that band the device's contracted float32 norm may fall on the other side: replay_ref.py)."""
    d = np.sqrt(np.sum((out["achieved_next"].astype(np.float64) - out["goal"].astype(np.float64)[:, None, :]) ** 2, axis=-1))
    valid = np.arange(d.shape[1])[None, :] < out["length"][:, None]
    return ~((np.abs(d - GEOFENCE) <= 1e-6) & valid).any(axis=1)


def check_against(got, want, where):
    for name in COPIED:
        assert same(got[name], want[name]), (where, name)
    L = got["obs"].shape[1]
    pad = np.arange(L)[None, :] >= got["length"][:, None]
    for name in seq.PER_STEP:
        a = got[name]
        assert not np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint8).reshape(a.shape[0], L, -1)[pad].any(), (where, name)
    clear = clear_samples(got)
    share = 1.0 - clear.mean()
    print(f"{where}: {int((~clear).sum())} of {clear.size} samples have a step within 1e-6 of the geofence ({share:.2e})")
    assert share <= 0.05, (where, share)
    for name in DERIVED:
        assert same(got[name][clear], want[name][clear]), (where, name)


@pytest.fixture(scope="module")
def main(models):
    """The 12-step loop of the main shape, run once, and every minibatch the tests read taken at its end."""
    from hsr_env_amd.sim import BatchSim
    m = models["cfg2"]
    sim = BatchSim(m, N)
    sim.set_episodes(cfg2_spec(m, limit=LIMIT))
    sim.reset_sampled()
    loop = Loop(sim, m.body_id("block0"), SUB, T, offsets=(0, 70))
    loop.begin()
    for _ in range(STEPS):
        loop.step()
    windows = {(L, her): sample_seq(loop, 0, 3, B, L, her) for L in LENS for her in HERS}
    single = {her: loop.sample(0, 3, B, her) for her in HERS}
    again = sample_seq(loop, 0, 3, B, 3, 0.5)
    other_draw = sample_seq(loop, 0, 4, B, 3, 0.5)
    shard = sample_seq(loop, 1, 3, B, 3, 0.5)
    yield dict(loop=loop, ring=loop.rings[0], windows=windows, single=single, again=again, other_draw=other_draw, shard=shard)
    loop.close()


@pytest.fixture(scope="module")
def second(models):
    """The second shape; before every env-step the block of every env is put somewhere else on the table (module docstring)."""
    from hsr_env_amd.sim import BatchSim
    m = models["cfg2"]
    sim = BatchSim(m, N)
    sim.set_episodes(cfg2_spec(m, limit=LIMIT2))
    sim.reset_sampled()
    loop = Loop(sim, m.body_id("block0"), SUB, T2)
    loop.begin()
    rng = np.random.default_rng(8)
    x = m.joint_qpos_addr("block0joint")[0]
    for _ in range(STEPS2):
        t, q, v = sim.get_state()
        sim.sync()
        q[:, x], q[:, x + 1] = rng.uniform(-0.09, 0.09, N), rng.uniform(-0.15, 0.15, N)
        sim.set_state(t, q, v)
        loop.step()
    got = {her: sample_seq(loop, 0, 6, B2, L2, her) for her in HERS}
    yield dict(loop=loop, ring=loop.rings[0], got=got)
    loop.close()


@pytest.mark.parametrize("L", LENS)
def test_windows_are_the_stated_function(main, L):
    for her in HERS:
        got = main["windows"][(L, her)]
        check_against(got, seq.sample_seq(main["ring"], 3, B, L, her, GAMMA), (L, her))
        assert got["length"].min() >= 1 and got["length"].max() == min(L, LIMIT)
        assert (got["length"] < L).any() == (L > 1)


def test_seq_len_one_is_sample_dev_bit_for_bit(main):
    """Device against device, all samples: the window of one step and hsr_replay_sample_dev with the same draw."""
    for her in HERS:
        one, want = main["windows"][(1, her)], main["single"][her]
        for name in ("obs", "action", "next_obs", "achieved_next", "reward", "done"):
            assert same(one[name][:, 0], want[name]), (her, name)
        assert same(one["goal"], want["goal"]) and same(one["index"], want["index"])
        assert np.all(one["length"] == 1) and np.all(one["nstep"] == 1)
        assert same(one["nstep_obs"], want["next_obs"]) and same(one["nstep_done"], want["done"])
        assert set(np.unique(want["reward"]).tolist()) <= {0.0, 1.0}
        assert same(one["nstep_return"], want["reward"]) and np.all(one["nstep_discount"] == np.float32(GAMMA))


def test_second_shape_and_its_coverage(second):
    """Windows cut by seq_len.  The cases are counted on the restatement's own output, so the comparison cannot pass by missing them."""
    ring = second["ring"]
    want = {her: seq.sample_seq(ring, 6, B2, L2, her, GAMMA) for her in HERS}
    w = want[1.0]
    counts = dict(middle=int(((1 < w["nstep"]) & (w["nstep"] < w["length"])).sum()),
                  at_end=int(((w["nstep"] == w["length"]) & (w["nstep_done"] == 1) & (w["length"] > 1)).sum()),
                  short=int((w["length"] < L2).sum()), not_done=int((want[0.0]["nstep_done"] == 0).sum()))
    by_age = ring.ep_id[ring.slot(np.arange(ring.count))].astype(np.int64)
    run_len = (by_age[:, None, :] == by_age[None, :, :]).sum(0)
    print(f"coverage {counts}; lengths {np.bincount(w['length']).tolist()}; episode runs in the ring up to {run_len.max()} steps")
    assert min(counts.values()) >= 10, counts
    assert run_len.max() > L2 and (w["length"] == L2).sum() >= 10            # cut by seq_len, not by the episode
    for her in HERS:
        check_against(second["got"][her], want[her], ("second", her))


def test_same_draw_same_bytes_and_a_shard_draws_its_own(main):
    base = main["windows"][(3, 0.5)]
    for name in seq.SEQ_FIELDS:
        assert same(main["again"][name], base[name]), name
    assert not same(main["other_draw"]["index"], base["index"])
    assert not same(main["shard"]["index"], base["index"])
    check_against(main["shard"], seq.sample_seq(main["loop"].rings[1], 3, B, 3, 0.5, GAMMA), "shard")


def test_every_output_may_be_null(main):
    loop, base = main["loop"], main["windows"][(3, 0.5)]
    for name in seq.SEQ_FIELDS:
        got = sample_seq(loop, 0, 3, B, 3, 0.5, skip=(name,))
        assert set(got) == set(seq.SEQ_FIELDS) - {name}
        for other, v in got.items():
            assert same(v, base[other]), (name, other)
    assert sample_seq(loop, 0, 3, B, 3, 0.5, skip=seq.SEQ_FIELDS) == {}
    loop.reps[0].sample_seq_dev(3, B, 3, 0.5, GAMMA, ReplaySeqOut())


def test_refused_calls_leave_no_trace(models):
    """Each refusal leaves the sentinel-filled outputs and the ring as they were; the ring is seen through a her_ratio = 0 minibatch."""
    from hsr_env_amd.sim import BatchSim
    m = models["cfg2"]
    bid = m.body_id("block0")
    sim = BatchSim(m, 9)
    sim.set_episodes(cfg2_spec(m, limit=LIMIT))
    sim.reset_sampled()
    cap = 3
    loop = Loop(sim, bid, SUB, cap, seed=1)
    rep, ring = loop.reps[0], loop.rings[0]
    t = sentinel_tensors(8, cap + 1, loop.od, sim.nu)

    def refuse(batch, L, her, gamma, out=True):
        with pytest.raises(AssertionError, match="hsr_replay_sample_seq_dev"):
            rep.sample_seq_dev(0, batch, L, her, gamma, struct_of(t) if out else None)
        sim.sync()
        for name, v in t.items():
            assert untouched(v), name

    refuse(8, 2, 0.5, GAMMA)                                    # an empty ring
    loop.begin()
    refuse(8, 2, 0.5, GAMMA)                                    # committed, still empty
    for _ in range(4):
        loop.step()
    sim.sample_ctrl_dev(4, loop.p("ctrl"))
    sim.step_dev(loop.p("ctrl"), SUB, bid, GEOFENCE, loop.p("obs"), loop.p("rew"), loop.p("done"), None)
    rep.record_dev(loop.p("ctrl"), loop.p("obs"), loop.p("rew"), loop.p("done"))
    refuse(8, 2, 0.5, GAMMA)                                    # a pending record
    assert rep.state() == (3, 1, 4)
    # the commit replaces the head row only; the pending transition closes with it, so take the restatement along
    final, rew, done, ctrl = loop.host("obs", "rew", "done", "ctrl")
    ring.record(ctrl, final, rew, done, sim.body_xpos(bid), sim.body_xpos(MOCAP_BODY))
    sim.episode_end_dev(loop.p("obs"), loop.p("rew"), loop.p("done"), None, loop.p("kind"), None, None)
    rep.commit_dev(loop.p("obs"), loop.p("kind"))
    after, kind = loop.host("obs", "kind")
    ring.commit(after, kind)
    assert rep.state() == (3, 2, 5)
    base = loop.sample(0, 3, 64, 0.0)
    refuse(8, 0, 0.5, GAMMA)
    refuse(8, -1, 0.5, GAMMA)
    refuse(8, cap + 1, 0.5, GAMMA)
    for gamma in (float("nan"), -0.1, 1.5, float("inf")):
        refuse(8, 2, 0.5, gamma)
    for her in (-0.01, 1.01, float("nan")):
        refuse(8, 2, her, GAMMA)
    refuse(0, 2, 0.5, GAMMA)
    refuse(8, 2, 0.5, GAMMA, out=False)                         # out == NULL
    assert rep.state() == (3, 2, 5)
    got, want = loop.sample(0, 3, 64, 0.0), ring.sample(3, 64, 0.0)
    for name in FIELDS:
        assert same(got[name], base[name]), name               # the refused calls left no trace: the same bytes as before them,
        assert same(got[name], want[name]), name               # and the ring is the one the valid calls alone built
    # and the call goes through once its numbers are in order: seq_len = capacity, gamma at both ends
    for gamma in (0.0, 1.0):
        check_against(sample_seq(loop, 0, 1, 8, cap, 0.5, gamma), seq.sample_seq(ring, 1, 8, cap, 0.5, gamma), ("edge", gamma))
    loop.close()


def test_env_surface_returns_the_ring_s_rows(models):
    m = models["cfg3"]
    env = VecHSREnv(model=m, goals=[GoalSpec("block0", GOAL, GEOFENCE)], starts={"block0joint": BLOCK_START}, steps_per_action=SUB, n_envs=5,
                    obs_type="openai", auto_reset=True, max_episode_steps=3)
    replay = env.make_replay(8, her_ratio=0.5)
    acted_on, terminal = [env.reset().copy()], []
    rng = np.random.default_rng(6)
    for _ in range(5):
        obs, _, _, info = env.step(rng.uniform(-1, 1, (5, m.nu)).astype(np.float32))
        acted_on.append(obs.copy()); terminal.append(info["terminal_observation"].copy())
    out = replay.sample_sequences(64, 3)
    env.sim.sync()
    dev = torch.device("cuda", 0)
    assert set(out) == set(seq.SEQ_FIELDS)
    for k, (shape, dtype) in shapes(64, 3, 25, m.nu).items():
        assert tuple(out[k].shape) == shape and out[k].dtype == dtype and out[k].device == dev, k
    host = {k: v.cpu().numpy() for k, v in out.items()}
    e, slot, length, n = host["index"][:, 0], host["index"][:, 1], host["length"], host["nstep"]
    assert np.all((1 <= length) & (length <= 3) & (1 <= n) & (n <= length)) and (length > 1).any()
    for i in range(64):
        for k in range(3):
            if k < length[i]:
                s = slot[i] + k                                # capacity 8, 5 steps: the slot is the env-step
                assert same(host["obs"][i, k], acted_on[s][e[i]]) and same(host["next_obs"][i, k], terminal[s][e[i]]), (i, k)
            else:
                assert not host["obs"][i, k].any() and not host["next_obs"][i, k].any() and not host["action"][i, k].any(), (i, k)
        assert same(host["nstep_obs"][i], terminal[slot[i] + n[i] - 1][e[i]]), i
    assert np.allclose(host["nstep_discount"], np.float32(0.99) ** n, rtol=1e-6)
    first = replay.sample(64)["index"].cpu().numpy()
    assert not np.array_equal(first, host["index"])            # one draw counter: sample() moved on from the windows' draw
    assert replay.sample_sequences(64, 3) is out                # tensors are cached per shape and overwritten
    env.close()
