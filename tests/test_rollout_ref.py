"""The numpy restatement of the on-policy rollout (tests/rollout_ref.py) against independent forms of what it restates: GAE against the fp64
closed form, the shuffle as a permutation.  No GPU."""
import numpy as np
import pytest

import rollout_ref as ref


def closed_form(reward, value, kind, v_term, last_value, gamma, lam, magnitudes=False):
    """adv_t = sum over k >= t inside t's episode of (gamma lam)^(k - t) delta_k, in fp64, term by term.  magnitudes: the same sum over the
    absolute values of everything that enters it - what a rounding error is relative to."""
    r, v, vt, lv = (np.asarray(x, np.float64) for x in (reward, value, v_term, last_value))
    g, gl = float(np.float32(gamma)), float(np.float32(np.float32(gamma) * np.float32(lam)))
    T, N = r.shape
    delta = np.zeros((T, N))
    for t in range(T):
        for e in range(N):
            nv = (lv[e] if t == T - 1 else v[t + 1, e]) if kind[t, e] == 0 else vt[t, e] if kind[t, e] == 2 else 0.0
            delta[t, e] = abs(r[t, e]) + g * abs(nv) + abs(v[t, e]) if magnitudes else r[t, e] + g * nv - v[t, e]
    adv = np.zeros((T, N))
    for t in range(T):
        for e in range(N):
            k, w = t, 1.0
            while True:
                adv[t, e] += w * delta[k, e]
                if kind[k, e] != 0 or k == T - 1:
                    break
                k, w = k + 1, w * gl
    return adv, adv + (np.abs(v) if magnitudes else v)


def signed_log_uniform(rng, shape):
    """Magnitudes in [1e-3, 1e3], either sign."""
    return (np.exp(rng.uniform(np.log(1e-3), np.log(1e3), shape)) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0), (0.0, 0.5)])
def test_gae_against_the_fp64_closed_form(gamma, lam):
    """Bound: 1e-5 relative to the largest magnitude that enters an advantage's sum.  A float32 operation errs by 2^-24 relative to its
    result; an advantage is a chain of at most 5 T = 60 operations on terms of magnitude <= the sum of the |terms| of its closed form, so the
    error stays below 60 x 2^-24 = 3.6e-6 of that sum."""
    rng = np.random.default_rng(11)
    T, N = 12, 40
    reward, value, v_term = (signed_log_uniform(rng, (T, N)) for _ in range(3))
    last_value = signed_log_uniform(rng, N)
    kind = rng.choice([0, 1, 2, 7], (T, N), p=[0.69, 0.15, 0.15, 0.01]).astype(np.uint8)
    kind[:, 0] = 0
    kind[:, 1] = 1
    adv, ret = ref.gae(reward, value, kind, v_term, last_value, gamma, lam)
    assert adv.dtype == np.float32 and ret.dtype == np.float32
    want_adv, want_ret = closed_form(reward, value, kind, v_term, last_value, gamma, lam)
    scale, scale_ret = closed_form(reward, value, kind, v_term, last_value, gamma, lam, magnitudes=True)
    assert np.all(scale >= np.abs(want_adv) * (1 - 1e-12))
    err_adv, err_ret = np.abs(adv - want_adv) / scale, np.abs(ret - want_ret) / scale_ret
    print(f"gamma {gamma} lam {lam}: largest relative error adv {err_adv.max():.2e}, ret {err_ret.max():.2e}")
    assert err_adv.max() <= 1e-5 and err_ret.max() <= 1e-5


def test_gae_edges_by_hand():
    """T = 3, one env per case, gamma = 0.5, lam = 0.5 (gl = 0.25): exact in float32."""
    reward = np.array([[1, 1, 1, 1], [2, 2, 2, 2], [4, 4, 4, 4]], np.float32)
    value = np.array([[8, 8, 8, 8], [16, 16, 16, 16], [32, 32, 32, 32]], np.float32)
    v_term = np.array([[0, 0, 0, 0], [0, 64, 64, 0], [0, 0, 0, 128]], np.float32)
    kind = np.array([[0, 0, 0, 0], [0, 2, 1, 0], [0, 0, 0, 2]], np.uint8)
    last = np.array([64, 64, 64, 64], np.float32)
    adv, ret = ref.gae(reward, value, kind, v_term, last, 0.5, 0.5)
    d2 = 4 + 0.5 * 64 - 32                     # 4: goes on at T-1, bootstraps from last_value
    d1 = 2 + 0.5 * 32 - 16                     # 2
    d0 = 1 + 0.5 * 16 - 8                      # 1
    assert adv[:, 0].tolist() == [d0 + 0.25 * (d1 + 0.25 * d2), d1 + 0.25 * d2, d2]
    assert adv[:, 1].tolist() == [d0 + 0.25 * (2 + 0.5 * 64 - 16), 2 + 0.5 * 64 - 16, d2]       # truncated at t = 1: v_term, no carry into it
    assert adv[:, 2].tolist() == [d0 + 0.25 * (2 - 16), 2 - 16, d2]                             # ended at t = 1: v_term ignored
    assert adv[:, 3].tolist() == [d0 + 0.25 * (d1 + 0.25 * (4 + 0.5 * 128 - 32)), d1 + 0.25 * (4 + 0.5 * 128 - 32), 4 + 0.5 * 128 - 32]
    assert np.array_equal(ret, adv + value)


@pytest.mark.parametrize("items", [1, 2, 3, 255, 256, 257, 350, 4096, 32769])
def test_perm_is_a_bijection(items):
    p = ref.perm(np.arange(items), items, seed=2 ** 35 + 9, epoch=3, env_offset=0)
    assert p.shape == (items,) and np.array_equal(np.sort(p), np.arange(items))
    h = ref.half_bits(items)
    assert items <= 4 ** h and (items == 1 or 4 ** h < 4 * items)


def test_perm_depends_on_epoch_and_shard_and_on_nothing_else():
    items, seed = 350, 2 ** 35 + 9
    base = ref.perm(np.arange(items), items, seed, 0, 0)
    assert np.array_equal(base, ref.perm(np.arange(items), items, seed, 0, 0))
    assert np.array_equal(base[100:150], ref.perm(np.arange(100, 150), items, seed, 0, 0))      # any piece can be produced alone
    for other in (ref.perm(np.arange(items), items, seed, 1, 0), ref.perm(np.arange(items), items, seed, 0, 70),
                  ref.perm(np.arange(items), items, seed + 1, 0, 0)):
        assert (other != base).sum() > items // 2
    assert not np.array_equal(base, np.arange(items))


def test_store_protocol():
    s = ref.Store(3, 2, 4, 1, 0.99, 0.95)
    z = np.zeros
    for call in (lambda: s.stage(z((3, 1)), z(3), z(3)), lambda: s.close(z(3), z(3), z((3, 4))), lambda: s.bootstrap(z(3)), lambda: s.finish(z(3)), s.next,
                 lambda: s.minibatch(0, 0, 1, False)):
        with pytest.raises(ref.OutOfOrder):
            call()
    s.begin(np.ones((3, 4)))
    with pytest.raises(ref.OutOfOrder):
        s.bootstrap(z(3))
    for t in range(2):
        s.stage(z((3, 1)), z(3), z(3))
        with pytest.raises(ref.OutOfOrder):
            s.stage(z((3, 1)), z(3), z(3))
        s.close(z(3) + t, z(3), np.full((3, 4), 2.0 + t))
        s.bootstrap(z(3))
        assert np.all(s.obs[t] == 1.0 + t) and (s.state, s.t) == (ref.READY, t + 1)
    with pytest.raises(ref.OutOfOrder):
        s.stage(z((3, 1)), z(3), z(3))
    s.finish(z(3))
    out = s.minibatch(0, 0, 6, True)
    assert sorted(map(tuple, out["index"].tolist())) == [(t, e) for t in range(2) for e in range(3)]
    for first, count in ((0, 0), (-1, 2), (5, 2), (0, 7)):
        with pytest.raises(ref.OutOfOrder):
            s.minibatch(0, first, count, False)
    s.next()
    assert (s.state, s.t) == (ref.READY, 0) and np.all(s.head == 3.0)
