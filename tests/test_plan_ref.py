"""tests/plan_ref.py - the numpy restatement of the device planner the GPU tests compare with - against independent statements of the same
rules: the rank rule against a brute-force sort, the fixed tree against math.fsum, the Irwin-Hall normal against its moments, candidate 0
against the clamped mean, the cost recursion, shift and reset against loops.  No GPU."""
import math

import numpy as np
import pytest

import plan_ref as ref

f32 = np.float32


def planted(rng, K):
    """Random costs on a coarse grid (ties), with infinities of both signs and NaNs planted."""
    c = (rng.integers(0, max(2, K // 3), K) * 0.25).astype(f32)
    for value in (np.inf, -np.inf, np.nan):
        c[rng.random(K) < 0.1] = value
    return c


@pytest.mark.parametrize("K", [2, 5, 64, 70, 1024])
def test_rank_rule_against_a_brute_force_sort(K):
    rng = np.random.default_rng(K)
    for trial in range(6):
        c = planted(rng, K) if trial else np.full(K, 1.5, f32)          # trial 0: all equal, the index alone decides
        if trial == 5:
            c[:] = np.nan                                               # none finite
        keys, finite = ref.cost_keys(c)
        assert np.array_equal(finite, np.isfinite(c)) and np.all(keys[~finite] == np.inf) and np.array_equal(keys[finite], c[finite])
        order = sorted(range(K), key=lambda k: (float(keys[k]), k))
        want = np.empty(K, int)
        want[order] = np.arange(K)
        assert np.array_equal(ref.ranks(keys), want)


@pytest.mark.parametrize("K", [2, 5, 64, 70, 1024])
def test_tree_sum_against_fsum(K):
    """Every addition of a chain of d additions errs by at most 2^-53 of its partial sum, itself at most (1 + 2^-53)^d sum|x|: the tree's
    result is within d 2^-53 (1 + 2^-53)^d sum|x| of the exact sum, d = ceil(K / 64) + 6."""
    rng = np.random.default_rng(100 + K)
    d = ref.tree_depth(K)
    assert d == -(-K // 64) + 6
    for scale in (1.0, 1e6, 1e-6):
        x = (rng.standard_normal(K) * scale).astype(f32).astype(np.float64)
        keep = rng.random(K) < 0.5
        leaves = np.where(keep, x, 0.0)
        got = float(ref.tree_sum(leaves))
        exact = math.fsum(leaves.tolist())
        bound = d * 2.0 ** -53 * (1 + 2.0 ** -53) ** d * math.fsum(np.abs(leaves).tolist())
        assert abs(got - exact) <= bound
    assert float(ref.tree_sum(np.arange(K, dtype=np.float64))) == K * (K - 1) / 2          # small whole numbers: exact in any order
    both = ref.tree_sum(np.stack([np.ones(K), np.arange(K, dtype=np.float64)]))            # leading axes are independent sums
    assert both.tolist() == [K, K * (K - 1) / 2]


def test_z_has_the_moments_of_a_standard_normal():
    """n = 2^16 draws.  z has mean 0 and variance 1 exactly (4 uniforms: variance 4 / 12, scaled by 3), so the sample mean has standard
    deviation 1 / sqrt(n); the sample variance has standard deviation sqrt((kurtosis - 1) / n) <= sqrt(2 / n), the kurtosis of an
    Irwin-Hall sum of four being 3 - 6 / (5 4) = 2.7 < 3.  Five standard deviations each; |z| <= 2 sqrt(3) always."""
    n = 2 ** 16
    P, K, H, nu = 2, 1024, 4, 8
    assert P * K * H * nu == n
    z = np.stack([ref.z_from_words(ref.plan_words(2 ** 40 + 7, 5, P, K, H, nu, call=3, it=1, h=h)) for h in range(H)])
    assert z.dtype == f32 and z.size == n
    z = z.astype(np.float64).ravel()
    assert abs(z.mean()) < 5 / math.sqrt(n)
    assert abs(z.var() - 1) < 5 * math.sqrt(2 / n)
    assert np.abs(z).max() <= 2 * math.sqrt(3)
    assert len(np.unique(z)) > n // 2
    # another call, iteration, step, group offset or seed: other draws
    base = ref.plan_words(9, 0, 1, 4, 3, 7, 0, 0, 0)
    for other in (ref.plan_words(9, 0, 1, 4, 3, 7, 1, 0, 0), ref.plan_words(9, 0, 1, 4, 3, 7, 0, 1, 0), ref.plan_words(9, 0, 1, 4, 3, 7, 0, 0, 1),
                  ref.plan_words(9, 1, 1, 4, 3, 7, 0, 0, 0), ref.plan_words(10, 0, 1, 4, 3, 7, 0, 0, 0)):
        assert not np.array_equal(base, other)
    # a group's draws do not depend on how many groups there are
    assert np.array_equal(ref.plan_words(9, 0, 3, 4, 3, 7, 2, 1, 2)[2], ref.plan_words(9, 2, 1, 4, 3, 7, 2, 1, 2)[0])
    assert np.all(ref.z_draws(9, 0, 3, 4, 3, 7, 2, 1, 2)[:, 0] == 0)


def test_candidate_zero_is_the_clamped_mean():
    rng = np.random.default_rng(3)
    P, K, H, nu = 3, 5, 3, 7
    lo, hi = ref.ctrl_range(np.array([[-1, 1], [-0.5, 0.25], [1e30, 1e30], [-np.inf, 2], [0.1, 0.3], [-2, np.nan], [-1e30, 0.5]]))
    assert lo.tolist() == [-1, -0.5, -1, -1, f32(0.1), -2, -1] and hi.tolist() == [1, 0.25, 1, 2, f32(0.3), 1, 0.5]
    mean = (rng.standard_normal((P, H, nu)) * 2).astype(f32)
    sigma = rng.random((P, H, nu)).astype(f32)
    for h in range(H):
        x = ref.sample(mean, sigma, ref.z_draws(1, 0, P, K, H, nu, 0, 0, h), h, lo, hi)
        assert x.dtype == f32 and x.shape == (P, K, nu)
        assert np.array_equal(x[:, 0].view(np.uint32), ref.clamp(mean[:, h], lo, hi).view(np.uint32))
        assert np.all(x >= lo) and np.all(x <= hi) and np.ptp(x[:, :, 0]) > 0
    m0, s0 = ref.reset_state(P, H, lo, hi, 0.5)
    assert np.all(m0[..., 4] == f32(0.1)) and np.all(m0[..., :4] == 0)   # zero is clamped into the range
    assert np.array_equal(s0[0, 0], (f32(0.5) * ((hi - lo) * f32(0.5)).astype(f32)).astype(f32))


def test_cost_recursion_shift_and_reset_against_loops():
    rng = np.random.default_rng(4)
    n, H, gamma = 9, 5, 0.5
    d = rng.random((H, n)).astype(f32)
    done = np.zeros((H, n), bool); done[2, 1] = done[0, 2] = done[4, 3] = True
    bad = np.zeros((H, n), bool); bad[1, 4] = bad[2, 1] = True           # env 1: bad and done in one step -> bad wins
    c = ref.Costs(n)
    for h in range(H):
        c.step(d[h], done[h], bad[h], h, gamma)
    for e in range(n):
        J, g, alive, reach = f32(0), f32(1), True, -1
        for h in range(H):
            if not alive:
                continue
            if bad[h, e]:
                J, alive = f32(np.inf), False
                continue
            J = f32(J + f32(g * d[h, e])); g = f32(g * f32(gamma))
            if done[h, e]:
                alive, reach = False, h
        assert (c.J[e], c.g[e], c.alive[e], c.reach[e]) == (J, g, alive, reach), e
    assert c.reach.tolist() == [-1, -1, 0, 4, -1, -1, -1, -1, -1] and np.isinf(c.J[[1, 4]]).all()
    c.add(np.full(n, np.nan, f32))
    assert np.isnan(c.J).all()
    P, nu = 3, 2
    lo, hi = np.array([-1, -2], f32), np.array([1, 2], f32)
    mean = rng.standard_normal((P, H, nu)).astype(f32); sigma = rng.random((P, H, nu)).astype(f32)
    m, s = ref.shift(mean, sigma, [1, 0, 1], lo, hi, 0.5)
    assert np.array_equal(m[1], mean[1]) and np.array_equal(s[1], sigma[1])
    for p in (0, 2):
        assert np.array_equal(m[p, :-1], mean[p, 1:]) and np.array_equal(m[p, -1], mean[p, -1])
        assert np.all(s[p] == np.array([0.5, 1.0], f32))
    m, s = ref.reset(mean, sigma, [0, 1, 0], lo, hi, 0.5)
    assert np.all(m[1] == 0) and np.all(s[1] == np.array([0.5, 1.0], f32)) and np.array_equal(m[[0, 2]], mean[[0, 2]]) and np.array_equal(s[[0, 2]], sigma[[0, 2]])


def test_update_refits_to_the_elites():
    rng = np.random.default_rng(5)
    H, nu, K = 2, 3, 70
    act = rng.standard_normal((H, nu, K)).astype(f32)
    J = rng.random(K).astype(f32)
    half = np.array([1, 1, 2], f32)
    mean, sigma = np.zeros((H, nu), f32), np.ones((H, nu), f32)
    m, s, elite, best, cost, failed = ref.update(mean, sigma, act, J, 7, 1.0, 0.05, half)
    top = np.argsort(J, kind="stable")[:7]
    assert failed == 0 and sorted(np.flatnonzero(elite)) == sorted(top) and best == top[0] and cost == J[top[0]]
    assert np.allclose(m, act[..., top].astype(np.float64).mean(-1), rtol=0, atol=1e-6)
    assert np.allclose(s, np.maximum(act[..., top].astype(np.float64).std(-1), 0.05 * half), rtol=0, atol=1e-6)
    # fewer finite costs than elites: E' = the finite ones; none: untouched and counted
    J2 = np.full(K, np.inf, f32); J2[[3, 40]] = [2.0, 1.0]
    m, s, elite, best, cost, failed = ref.update(mean, sigma, act, J2, 7, 0.5, 0.05, half)
    assert failed == 0 and np.flatnonzero(elite).tolist() == [3, 40] and best == 40 and cost == 1.0
    assert np.allclose(m, 0.5 * act[..., [3, 40]].astype(np.float64).mean(-1), rtol=0, atol=1e-6)
    m, s, elite, best, cost, failed = ref.update(mean, sigma, act, np.full(K, np.nan, f32), 7, 0.5, 0.05, half)
    assert failed == 1 and not elite.any() and best == 0 and np.isinf(cost) and m is not mean and np.array_equal(m, mean) and np.array_equal(s, sigma)
