"""The running-moments normaliser on the device (hsr_env_amd/normalize.py; csrc/normalize.h) against the fp64 restatement of
tests/normalize_ref.py: the moments after any sequence of updates, rows left out, no-ops, reproducibility, the float32 apply, and the
wiring into VecHSREnv's device loop and the replay's samplers.

THE BOUND.  u = 2^-53 is fp64's unit roundoff.  A column of M counted rows, merged in U updates, with mag = mean|x|:
  mean.  A batch sum of m values in any order is off by at most (m - 1) u sum|x|, its mean by about m u mag; a Chan merge adds four
    roundings of a quantity no larger than the column's values (delta, delta m, / tot, the addition), and a merged mean is a convex
    combination of batch means, so their errors do not add up beyond the largest.  The device is therefore within (M + 8 U) u mag of the
    exact mean; the two-pass numpy reference, itself a sum of M values, within M u mag.  Used: b_mean = (M + 8 U) 2^-52 mag, twice the
    device's share, in the manner of stats_bound of tests/test_gpu_rollout.py.
  m2.  The sums of squares are sums of positive terms, each with three roundings: relative error (M + 8 U) 2^-52 at most, on either side.
    The mean's error e enters in two places: a batch's sum((x - mean_b - e)^2) = m2_b + m e^2 exactly (the cross term vanishes), and
    Chan's cross term delta^2 count m / tot, whose weight is at most m and whose delta is at most the column's span:
    2 span e m + e^2 m per merge, M (2 span e + e^2) over all of them, with e <= b_mean.
    Used: b_m2 = (M + 8 U) 2^-52 m2 + M (2 span b_mean + b_mean^2).
The bounds come from the number format and the shapes alone.  Every case asserts that they stay below 1e-3 of the column's std (of m2 for
b_m2): a float32 accumulator, a sum of x^2 without a shift, or a wrong merge formula is orders of magnitude outside them.
"""
import numpy as np
import pytest
import torch        # before the library: torch's HIP runtime must be the first one loaded into the process (as in test_gpu_episodes.py)

import normalize_ref as ref
from hsr_env_amd.env import GoalSpec, VecHSREnv
from hsr_env_amd.normalize import ObsNormalizer, RunningNorm
from test_gpu_episodes import BLOCK_START, GEOFENCE, GOAL, SEED

pytestmark = pytest.mark.gpu
DIMS, NS = (1, 3, 25, 27, 53), (1, 63, 64, 65, 257, 4099)
OFFSETS, SCALES = (0.0, 3.0, -40.0, 1000.0), (1.0, 0.01, 5.0, 0.01)
EPS32 = float(np.float32(0.01))


@pytest.fixture(scope="module")
def sim(models):
    from hsr_env_amd.sim import BatchSim
    s = BatchSim(models["cfg2"], 70)
    yield s
    s.close()


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def make_rows(rng, n, dim, offset=None, scale=None):
    off = np.array([OFFSETS[c % 4] for c in range(dim)]) if offset is None else offset
    sc = np.array([SCALES[c % 4] for c in range(dim)]) if scale is None else scale
    return (off + sc * rng.standard_normal((n, dim))).astype(np.float32)


def bounds(updates, dim):
    """updates [(rows, mask or None), ..] -> (count, mean, m2, skipped) of the reference and (b_mean, b_m2) as derived above."""
    count, mean, m2, skipped = ref.moments(updates, dim)
    if count == 0:
        return (count, mean, m2, skipped), np.zeros(dim), np.zeros(dim)
    x = np.concatenate([ref.counted(r, m)[0].reshape(-1, dim) for r, m in updates])
    k = (count + 8 * len(updates)) * 2.0 ** -52
    b_mean = k * np.abs(x).mean(axis=0)
    span = x.max(axis=0) - x.min(axis=0)
    b_m2 = k * m2 + count * (2 * span * b_mean + b_mean * b_mean)
    return (count, mean, m2, skipped), b_mean, b_m2


def check_state(norm, updates, dim, floor=0.0):
    """The device's fp64 state against the reference of all counted rows, within the derived bounds - and the bounds within 1e-3 of the
    column's std.  floor: only for a column that is constant over all counted rows (m2 == 0 in the reference: an env's mocap quaternion,
    say), which has no std to compare with; the std the normaliser uses for it is eps, and the bound is held against that.  Prints the
    figures."""
    (count, mean, m2, skipped), b_mean, b_m2 = bounds(updates, dim)
    got_count, got_mean, got_m2, got_skipped = norm.state()
    assert got_count == count and got_skipped == skipped, (got_count, count, got_skipped, skipped)
    if count == 0:
        assert not got_mean.any() and not got_m2.any()
        return
    std = np.sqrt(m2 / count)
    e_mean, e_m2 = np.abs(got_mean - mean), np.abs(got_m2 - m2)
    const = m2 == 0
    std_used, m2_used = np.where(const, floor, std), np.where(const, count * floor * floor, m2)
    with np.errstate(divide="ignore", invalid="ignore"):
        print(f"dim {dim} M {int(count)} U {len(updates)}, {int(const.sum())} constant column(s): max |mean err| / std "
              f"{np.max(e_mean / std_used):.2e} (bound / std {np.max(b_mean / std_used):.2e}), max |m2 err| / m2 "
              f"{np.nanmax(e_m2 / m2_used):.2e} (bound / m2 {np.max(b_m2 / m2_used):.2e})")
    assert (b_mean < 1e-3 * std_used).all() and (b_m2 < 1e-3 * m2_used).all(), (b_mean / std_used, b_m2 / m2_used)
    assert (e_mean <= b_mean).all(), (e_mean, b_mean)
    assert (e_m2 <= b_m2).all(), (e_m2, b_m2)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def check_published(norm, eps=EPS32):
    """The published vectors are the publish rule of the device's own fp64 state: mean32 exactly, rstd32 within one float32 ulp (the
    device's fp64 sqrt and division may differ from numpy's in their last bit, which float32 rounding can carry over)."""
    count, mean, m2, _ = norm.state()
    mean32, rstd32 = (t.cpu().numpy() for t in norm.published())
    want_mean, want_rstd = ref.publish(count, mean, m2, eps)
    assert np.array_equal(mean32, want_mean)
    assert (np.abs(rstd32.astype(np.float64) - want_rstd) <= ulp32(want_rstd)).all()
    return mean32, rstd32


def bits(a):
    """A float array as its bit patterns; arrays of other kinds as they are."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    """Bit for bit; NaNs match NaNs (their payload is the platform's)."""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def same_state(s, t):
    return s[0] == t[0] and s[3] == t[3] and np.array_equal(bits(s[1]), bits(t[1])) and np.array_equal(bits(s[2]), bits(t[2]))


def pattern_mask(n, k):
    m = ((np.arange(n) + k) % 3 != 1).astype(np.uint8)
    m[0] = 1
    return m


@pytest.mark.parametrize("dim", DIMS)
def test_moments(sim, dim):
    """Three updates of n rows for every n at which the tiling changes (one lane, a wave short of one, full, one more, three tiles with a
    ragged last one, 33 tiles): without a mask (contiguous rows), with one (rows strided inside a wider tensor), with an all-zero one."""
    rng = np.random.default_rng(100 + dim)
    for n in NS:
        data = [make_rows(rng, n, dim) for _ in range(3)]
        plain, masked, none = (RunningNorm(sim, dim) for _ in range(3))
        ups_plain, ups_masked = [], []
        for k, rows in enumerate(data):
            plain.update(dev(rows))
            ups_plain.append((rows, None))
            wide = torch.full((n, dim + 5), float("nan"), device="cuda")
            wide[:, 2:2 + dim] = dev(rows)
            mask = pattern_mask(n, k)
            masked.update(wide[:, 2:2 + dim], dev(mask, torch.uint8))
            ups_masked.append((rows, mask))
            none.update(dev(rows), dev(np.zeros(n), torch.uint8))
        check_state(plain, ups_plain, dim)
        check_state(masked, ups_masked, dim)
        check_published(plain)
        assert none.state()[0] == 0 and not none.state()[1].any() and not none.state()[2].any() and none.state()[3] == 0
        m32, r32 = (t.cpu().numpy() for t in none.published())
        assert np.array_equal(m32, np.zeros(dim, np.float32)) and np.array_equal(r32, np.ones(dim, np.float32))
        for r in (plain, masked, none):
            r.close()


@pytest.mark.parametrize("dim", (65, 130))
def test_moments_of_rows_wider_than_a_tile(sim, dim):
    """More than 64 columns: the workgroup walks the columns in pieces, and a row is left out for a NaN in any of them."""
    rng = np.random.default_rng(dim)
    for n in (65, 257):
        rows = [make_rows(rng, n, dim) for _ in range(2)]
        rows[1][n // 2, dim - 1] = np.nan
        rows[1][n - 1, 64] = np.inf
        norm = RunningNorm(sim, dim)
        ups = []
        for k, r in enumerate(rows):
            mask = pattern_mask(n, k)
            mask[n - 1] = 1
            norm.update(dev(r), dev(mask, torch.uint8))
            ups.append((r, mask))
        check_state(norm, ups, dim)
        assert norm.skipped == 1 + int(pattern_mask(n, 1)[n // 2])
        norm.close()


def test_cancellation(sim):
    """Offset 1000, scale 0.01 (float32 still resolves the spread): 200 updates of 70 rows, and the same rows in one update of 14 000.
    A float32 accumulator or a sum of x^2 fails here by orders of magnitude."""
    rng = np.random.default_rng(7)
    dim = 27
    rows = make_rows(rng, 14000, dim, offset=1000.0, scale=0.01)
    many, one = RunningNorm(sim, dim, eps=1e-3), RunningNorm(sim, dim)         # (the default eps = 0.01 would floor this std away)
    all_dev = dev(rows)
    for k in range(200):
        many.update(all_dev[70 * k:70 * (k + 1)])
    one.update(all_dev)
    check_state(many, [(rows[70 * k:70 * (k + 1)], None) for k in range(200)], dim)
    check_state(one, [(rows, None)], dim)
    mean32, rstd32 = check_published(many, eps=1e-3)
    std = rows.astype(np.float64).std(axis=0)
    assert np.allclose(1.0 / rstd32, std, rtol=1e-6, atol=0) and (std > 0.009).all() and (std < 0.011).all()
    many.close(); one.close()


def test_nonfinite_rows_are_left_out_in_place(sim):
    """NaN and +-inf planted in known rows and columns: the state equals, bit for bit, that of the run where a mask leaves those rows
    out of clean data - a row that is left out adds +0.0 in the place of its value, whatever it held.  skipped counts them."""
    rng = np.random.default_rng(11)
    dim, n = 27, 257
    planted = [(0, 0, np.nan), (63, 13, np.inf), (64, 26, -np.inf), (127, 5, np.nan), (128, 0, np.inf), (200, 26, np.nan), (256, 13, -np.inf), (256, 14, np.nan)]
    rows_hit = sorted({r for r, _, _ in planted})
    dirty, clean = RunningNorm(sim, dim), RunningNorm(sim, dim)
    ups = []
    for k in range(2):
        rows = make_rows(rng, n, dim)
        bad = rows.copy()
        for r, c, v in planted:
            bad[r, c] = v
        mask = np.ones(n, np.uint8)
        mask[rows_hit] = 0
        dirty.update(dev(bad))
        clean.update(dev(rows), dev(mask, torch.uint8))
        ups.append((bad, None))
    sd, sc = dirty.state(), clean.state()
    assert sd[3] == 2 * len(rows_hit) and sc[3] == 0
    assert sd[0] == sc[0] == 2 * (n - len(rows_hit))
    assert np.array_equal(bits(sd[1]), bits(sc[1])) and np.array_equal(bits(sd[2]), bits(sc[2]))
    assert all(same(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(dirty.published(), clean.published()))
    check_state(dirty, ups, dim)
    # a row the mask does not select is not looked at: neither counted nor skipped
    dirty.update(dev(bad), dev(mask, torch.uint8))
    assert dirty.skipped == 2 * len(rows_hit) and dirty.count == 3 * (n - len(rows_hit))
    dirty.close(); clean.close()


def test_noops_leave_every_bit(sim):
    rng = np.random.default_rng(13)
    dim = 25
    norm = RunningNorm(sim, dim)
    norm.update(dev(make_rows(rng, 65, dim)))
    before, pub = norm.state(), [t.cpu().numpy().copy() for t in norm.published()]
    rows = dev(make_rows(rng, 257, dim))
    norm.update(rows, dev(np.zeros(257), torch.uint8))          # an all-zero mask
    norm.update(rows[:0])                                       # no rows at all
    norm.update(torch.zeros((0, dim), device="cuda"), torch.zeros(0, dtype=torch.uint8, device="cuda"))
    assert same_state(norm.state(), before)
    assert all(np.array_equal(bits(a), bits(b.cpu().numpy())) for a, b in zip(pub, norm.published()))
    allnan = torch.full((64, dim), float("nan"), device="cuda")  # m == 0 with rows selected: the moments stay, skipped counts
    norm.update(allnan)
    after = norm.state()
    assert after[0] == before[0] and np.array_equal(bits(after[1]), bits(before[1])) and np.array_equal(bits(after[2]), bits(before[2]))
    assert after[3] == before[3] + 64
    assert all(np.array_equal(bits(a), bits(b.cpu().numpy())) for a, b in zip(pub, norm.published()))
    norm.close()


def test_reproducible_and_resumable(sim):
    rng = np.random.default_rng(17)
    dim = 27
    seq = [(make_rows(rng, n, dim), pattern_mask(n, k) if k % 2 else None) for k, n in enumerate((70, 257, 64, 4099, 65))]
    seq[3][0][17, 3] = np.nan

    def run(norm, part):
        for rows, mask in part:
            norm.update(dev(rows), None if mask is None else dev(mask, torch.uint8))
        return norm

    a, b = run(RunningNorm(sim, dim), seq), run(RunningNorm(sim, dim), seq)
    assert same_state(a.state(), b.state())
    half = run(RunningNorm(sim, dim), seq[:2])
    resumed = RunningNorm(sim, dim)
    resumed.load_state_dict(half.state_dict())
    assert same_state(resumed.state(), half.state())
    assert all(np.array_equal(bits(x.cpu().numpy()), bits(y.cpu().numpy())) for x, y in zip(resumed.published(), half.published()))
    run(resumed, seq[2:])
    assert same_state(resumed.state(), a.state()) and a.skipped == 1
    assert all(np.array_equal(bits(x.cpu().numpy()), bits(y.cpu().numpy())) for x, y in zip(resumed.published(), a.published()))
    # merge_states of two device states is Chan's rule on the host: the moments of both parts together
    tail = run(RunningNorm(sim, dim), seq[2:])
    merged = RunningNorm.merge_states([half.state_dict(), tail.state_dict()])
    fresh = RunningNorm(sim, dim)
    fresh.load_state_dict(merged)
    check_state(fresh, seq, dim)
    with pytest.raises(AssertionError, match="count negative"):
        fresh.load_state_dict({**merged, "count": -1.0})
    with pytest.raises(AssertionError, match="m2 negative"):
        fresh.load_state_dict({**merged, "m2": -merged["m2"] - 1.0})
    a.clear()
    assert a.state()[0] == 0 and not a.state()[1].any() and a.skipped == 0
    for r in (a, b, half, resumed, tail, fresh):
        r.close()


def test_argument_checks(sim):
    for bad in (dict(dim=0), dict(dim=1025), dict(eps=0.0), dict(eps=-1.0), dict(clip=0.0), dict(clip=float("inf")), dict(clip=float("nan"))):
        with pytest.raises(AssertionError, match="hsr_batch_norm_create"):
            RunningNorm(sim, **{**dict(dim=3, eps=0.01, clip=5.0), **bad})
    norm = RunningNorm(sim, 3)
    rows = torch.zeros((8, 3), device="cuda")
    with pytest.raises(AssertionError, match="n < 0"):
        norm._norm.update_dev(rows.data_ptr(), 3, None, -1)
    with pytest.raises(AssertionError, match="stride below dim"):
        norm._norm.update_dev(rows.data_ptr(), 2, None, 8)
    with pytest.raises(AssertionError, match="stride below dim"):
        norm._norm.apply_dev(rows.data_ptr(), 3, rows.data_ptr(), 2, 8)
    assert norm.count == 0
    norm.close()


def test_apply(sim):
    rng = np.random.default_rng(19)
    dim, n = 27, 257
    norm = RunningNorm(sim, dim)
    norm.update(dev(make_rows(rng, 4099, dim)))
    mean32, rstd32 = check_published(norm)
    x = make_rows(rng, n, dim)
    x[3, 4] = np.nan; x[5, 0] = np.inf; x[6, 26] = -np.inf; x[7, :] = 1e30; x[8, :] = -1e30; x[9, :] = -0.0
    want = ref.apply(x, mean32, rstd32, 5.0)
    out = norm.apply(dev(x))
    assert same(out.cpu().numpy(), want)                        # out of place
    assert np.isnan(want[3, 4]) and (want[7] == 5.0).all() and (want[8] == -5.0).all() and want[5, 0] == 5.0 and want[6, 26] == -5.0
    assert np.abs(want[~np.isnan(want)]).max() == 5.0
    inplace = dev(x)
    assert norm.apply(inplace, out=inplace) is inplace and same(inplace.cpu().numpy(), want)
    wide_in, wide_out = torch.full((n, dim + 3), 7.0, device="cuda"), torch.full((n, dim + 6), -7.0, device="cuda")
    wide_in[:, 1:1 + dim] = dev(x)
    norm.apply(wide_in[:, 1:1 + dim], out=wide_out[:, 4:4 + dim])
    got = wide_out.cpu().numpy()
    assert same(got[:, 4:4 + dim], want) and (got[:, :4] == -7.0).all() and (got[:, 4 + dim:] == -7.0).all()
    assert same(norm.apply(dev(x).reshape(n, 1, dim)).cpu().numpy().reshape(n, dim), want)         # any leading shape
    assert same(norm.apply(x), want)                            # host rows: up, apply, down
    host_out = np.full_like(x, 9.0)
    assert norm.apply(x, out=host_out) is host_out and same(host_out, want)
    with pytest.raises(AssertionError, match="out for host rows"):
        norm.apply(x, out=np.zeros((n, dim), np.float64))
    # clipping holds at +-clip exactly with a clip of one's own
    tight = RunningNorm(sim, dim, eps=0.5, clip=0.25)
    tight.update(dev(x[10:]))
    m2_, r2_ = check_published(tight, eps=0.5)
    y = tight.apply(dev(x)).cpu().numpy()
    assert same(y, ref.apply(x, m2_, r2_, 0.25)) and np.abs(y[~np.isnan(y)]).max() == 0.25
    # nothing counted: the identity up to the clip
    empty = RunningNorm(sim, dim)
    ident = empty.apply(dev(x)).cpu().numpy()
    assert same(ident, ref.apply(x, np.zeros(dim, np.float32), np.ones(dim, np.float32), 5.0))
    small = np.abs(x) < 5.0
    assert np.array_equal(bits(ident[small]), bits(x[small]))
    # the eps floor on a constant column
    const = RunningNorm(sim, 3)
    rows = make_rows(rng, 70, 3)
    rows[:, 1] = 1000.0
    const.update(dev(rows))
    m32, r32 = check_published(const)
    assert m32[1] == np.float32(1000.0) and abs(float(r32[1]) - 1.0 / EPS32) <= ulp32(1.0 / EPS32) and const.state()[2][1] == 0.0
    assert np.array_equal(const.std, np.sqrt(np.maximum(const.state()[2] / 70, EPS32 ** 2))) and const.std[1] == EPS32
    probe = np.float32([[0.0, 1000.0, 0.0], [0.0, 1000.02, 0.0], [0.0, 999.0, 0.0]])
    y = const.apply(dev(probe)).cpu().numpy()
    assert same(y, ref.apply(probe, m32, r32, 5.0)) and y[0, 1] == 0.0 and 1.9 < y[1, 1] < 2.1 and y[2, 1] == -5.0
    for r in (norm, tight, empty, const):
        r.close()


# ---------------------------------------------------------------------------------------------------------------- the env and the replay
N_ENVS, LIMIT, STEPS, SUB, RING = 70, 3, 6, 20, 7


def drive(models, with_normalizer):
    """cfg2, 70 envs, time limit 3: reset, a replay, (a normaliser,) six env-steps of actions sampled on the device."""
    m = models["cfg2"]
    env = VecHSREnv(model=m, goals=[GoalSpec("block0", GOAL, GEOFENCE)], starts={"block0joint": BLOCK_START}, steps_per_action=SUB, n_envs=N_ENVS,
                    auto_reset=True, max_episode_steps=LIMIT)
    env.seed(SEED)
    env.reset()
    replay = env.make_replay(RING)
    nz = env.make_normalizer() if with_normalizer else None
    log = dict(first=env.state_vector().copy(), steps=[], policy=[], published=[])
    if nz is not None:
        env.sim.sync()
        log["policy"].append(nz.policy_obs.cpu().numpy())
        log["published"].append([t.cpu().numpy().copy() for t in nz.obs.published()])
    for _ in range(STEPS):
        obs, rew, done, info = env.step(env.sample_action_dev())
        log["steps"].append((obs.copy(), np.asarray(rew).copy(), np.asarray(done).copy(), np.asarray(info["substeps"]).copy()))
        if nz is not None:
            log["policy"].append(nz.policy_obs.cpu().numpy())
            log["published"].append([t.cpu().numpy().copy() for t in nz.obs.published()])
    return env, replay, nz, log


@pytest.fixture(scope="module")
def wired(models):
    with_nz, without = drive(models, True), drive(models, False)
    yield with_nz, without
    with_nz[0].close(); without[0].close()


def test_env_counts_every_policy_row_once(wired):
    (env, replay, nz, log), _ = wired
    od = env.obs_dim
    assert nz.policy_obs.shape == (N_ENVS, od) and isinstance(nz, ObsNormalizer) and nz.goal.dim == 3
    assert nz.obs.count == N_ENVS * (1 + STEPS) and nz.obs.skipped == 0
    ups = [(log["first"], None)] + [(s[0], None) for s in log["steps"]]
    # policy_obs is the apply of the rows the env returned, with the statistics that include them
    for rows, policy, (mean32, rstd32) in zip([u[0] for u in ups], log["policy"], log["published"]):
        assert same(policy, ref.apply(rows, mean32, rstd32, 5.0))
    # a masked reset counts exactly the masked rows, and normalises all of them
    mask = np.zeros(N_ENVS, bool)
    mask[[1, 5, 64, 69]] = True
    obs = env.reset(mask)
    assert nz.obs.count == N_ENVS * (1 + STEPS) + 4
    ups.append((obs, mask))
    mean32, rstd32 = (t.cpu().numpy() for t in nz.obs.published())
    assert same(nz.policy_obs.cpu().numpy(), ref.apply(obs, mean32, rstd32, 5.0))
    check_state(nz.obs, ups, od, floor=EPS32)
    check_published(nz.obs)
    # a jump is not an observation: fork() leaves the statistics alone, and policy_obs follows the rows
    before = nz.obs.state()
    env.fork(0, 1)
    assert same_state(nz.obs.state(), before)
    policy = nz.policy_obs.cpu().numpy()
    assert same(policy[1], policy[0]) and same(policy, ref.apply(env.state_vector(), mean32, rstd32, 5.0))
    with pytest.raises(ValueError, match="already feeds a normaliser"):
        env.make_normalizer()


def test_env_results_and_samples_do_not_change(wired):
    """Before the masked reset and the fork of the test above touched the first env, both ran the same steps: same bits."""
    (_, _, _, log), (_, _, none, plain) = wired
    assert none is None and same(log["first"], plain["first"])
    for a, b in zip(log["steps"], plain["steps"]):
        assert all(same(x, y) if x.dtype.kind == "f" else np.array_equal(x, y) for x, y in zip(a, b))


def test_replay_samples_normalised_on_read(models):
    (env, replay, nz, _), (twin, twin_replay, _, _) = drive(models, True), drive(models, False)
    raw0, twin0 = replay.sample(64), twin_replay.sample(64)
    env.sim.sync(); twin.sim.sync()
    for k in raw0:
        assert same(raw0[k].cpu().numpy(), twin0[k].cpu().numpy()), k                      # an attached normaliser changes no sample
    nz.update_goals(raw0)
    assert nz.goal.count == 64
    goal_ref = ref.moments([(raw0["goal"].cpu().numpy(), None)], 3)
    assert np.abs(nz.goal.mean - goal_ref[1]).max() < 1e-12
    # sample(normalizer=nz) = apply_batch of the raw sample of the same draw
    got = {k: v.cpu().numpy() for k, v in replay.sample(64, normalizer=nz).items()}
    raw = twin_replay.sample(64)
    twin.sim.sync()
    raw_host = {k: v.cpu().numpy() for k, v in raw.items()}
    want = {k: v.cpu().numpy() for k, v in nz.apply_batch({k: v.clone() for k, v in raw.items()}).items()}
    pub = {0: [t.cpu().numpy() for t in nz.obs.published()], 1: [t.cpu().numpy() for t in nz.goal.published()]}
    for k in got:
        assert same(got[k], want[k]), k
        which = 0 if k in ObsNormalizer.OBS_KEYS else 1 if k in ObsNormalizer.GOAL_KEYS else None
        if which is None:
            assert same(got[k], raw_host[k]), k
        else:
            assert same(got[k], ref.apply(raw_host[k], *pub[which], 5.0)) and not same(got[k], raw_host[k]), k
    # windows: every row below its window's length is normalised, every row past it stays zero
    L = 4
    got = {k: v.cpu().numpy() for k, v in replay.sample_sequences(32, L, normalizer=nz).items()}
    raw = twin_replay.sample_sequences(32, L)
    twin.sim.sync()
    raw_host = {k: v.cpu().numpy() for k, v in raw.items()}
    length = raw_host["length"]
    assert (length < L).all() and (length >= 1).all()                                      # the time limit is 3: every window has padding
    live = np.arange(L)[None, :] < length[:, None]
    for k in got:
        which = 0 if k in ObsNormalizer.OBS_KEYS else 1 if k in ObsNormalizer.GOAL_KEYS else None
        if which is None:
            assert same(got[k], raw_host[k]), k
        elif got[k].ndim == 3:
            assert same(got[k][live], ref.apply(raw_host[k][live], *pub[which], 5.0)), k
            assert not got[k][~live].any() and not bits(got[k][~live]).any(), k
        else:
            assert same(got[k], ref.apply(raw_host[k], *pub[which], 5.0)), k
    env.close(); twin.close()


def test_env_with_the_openai_observation(models):
    """The same wiring for the 25-float observation, with nothing else attached: the loop reads the policy rows on the device for the
    normaliser alone.  70 envs, time limit 3, six env-steps of 20 substeps - on cfg3, the smallest model with the finger joints this
    observation needs (cfg2 has none, and the env refuses obs_type='openai' for it)."""
    m = models["cfg3"]
    env = VecHSREnv(model=m, goals=[GoalSpec("block0", GOAL, GEOFENCE)], starts={"block0joint": BLOCK_START}, steps_per_action=SUB, n_envs=N_ENVS,
                    obs_type="openai", auto_reset=True, max_episode_steps=LIMIT)
    env.seed(SEED)
    env.reset()
    nz = env.make_normalizer()
    assert nz.obs.dim == 25 and nz.policy_obs.shape == (N_ENVS, 25) and nz.obs.count == N_ENVS

    def policy_is_apply_of(rows):
        mean32, rstd32 = (t.cpu().numpy() for t in nz.obs.published())
        return same(nz.policy_obs.cpu().numpy(), ref.apply(rows, mean32, rstd32, 5.0))

    ups = [(env.state_vector().copy(), None)]
    assert policy_is_apply_of(ups[0][0])
    for _ in range(STEPS):
        obs, _, _, _ = env.step(env.sample_action_dev())
        ups.append((obs.copy(), None))
        assert policy_is_apply_of(obs)
    assert nz.obs.count == N_ENVS * (1 + STEPS) and nz.obs.skipped == 0
    mask = np.zeros(N_ENVS, bool)
    mask[[0, 7, 63, 64, 69]] = True
    obs = env.reset(mask)
    ups.append((obs, mask))
    assert nz.obs.count == N_ENVS * (1 + STEPS) + 5 and policy_is_apply_of(obs)
    check_state(nz.obs, ups, 25, floor=EPS32)
    check_published(nz.obs)
    env.close()
    with pytest.raises(ValueError, match="auto_reset"):
        VecHSREnv(model=m, n_envs=5).make_normalizer()


def test_count_does_not_depend_on_what_is_attached_when(models):
    """make_replay and make_rollout commit the current rows to what they attach; those rows were handed to the policy - and counted -
    before, so a normaliser attached first counts them once all the same, as does one attached last."""
    m = models["cfg2"]
    kw = dict(model=m, goals=[GoalSpec("block0", GOAL, GEOFENCE)], starts={"block0joint": BLOCK_START}, steps_per_action=5, n_envs=N_ENVS,
              auto_reset=True, max_episode_steps=LIMIT)
    states = []
    for normalizer_first in (True, False):
        env = VecHSREnv(**kw)
        env.seed(SEED)
        env.reset()
        nz = env.make_normalizer() if normalizer_first else None
        replay = env.make_replay(RING)
        rollout = env.make_rollout(4)
        nz = nz or env.make_normalizer()
        assert nz.obs.count == N_ENVS
        zeros = torch.zeros(N_ENVS, device="cuda")
        for k in range(2):
            rollout.stage(env.sample_action_dev(), zeros, zeros)
            env.step(env.sample_action_dev())
            assert nz.obs.count == N_ENVS * (k + 2) and replay.state()[0] == k + 1
        env.reset(np.arange(N_ENVS) < 3)
        assert nz.obs.count == N_ENVS * 3 + 3
        states.append((nz.obs.state(), nz.policy_obs.cpu().numpy()))
        env.close()
    assert same_state(states[0][0], states[1][0]) and same(states[0][1], states[1][1])


def test_attaching_does_not_disturb_a_rollout(models):
    """A rollout that is already fed keeps its head rows and its state when a normaliser joins it (25-float rows: the two share the
    loop's policy rows), and the step closes the one and feeds the other."""
    m = models["cfg3"]
    n = 5
    env = VecHSREnv(model=m, goals=[GoalSpec("block0", GOAL, GEOFENCE)], starts={"block0joint": BLOCK_START}, steps_per_action=5, n_envs=n,
                    obs_type="openai", auto_reset=True, max_episode_steps=2)
    env.reset()
    rollout = env.make_rollout(4)
    head, state = rollout.obs, rollout.state()
    before = head.cpu().numpy()
    nz = env.make_normalizer()
    assert rollout.obs is head and rollout.state() == state and same(head.cpu().numpy(), before)
    assert nz.obs.count == n
    zeros = torch.zeros(n, device="cuda")
    for k in range(2):
        rollout.stage(env.sample_action_dev(), zeros, zeros)
        obs, _, _, _ = env.step(env.sample_action_dev())
        assert rollout.state() == (1, k + 1) and nz.obs.count == n * (k + 2)
        mean32, rstd32 = (t.cpu().numpy() for t in nz.obs.published())
        assert same(rollout.obs.cpu().numpy(), obs) and same(nz.policy_obs.cpu().numpy(), ref.apply(obs, mean32, rstd32, 5.0))
    env.close()
