"""Self-test of the numpy restatement of the replay's priorities (tests/replay_prio_ref.py), on the CPU: the sampler draws cells in
proportion to their priorities, the descent never ends on a leaf without priority, updates follow the clamp, duplicate and staleness
rules, and new transitions enter with p_new.  No GPU."""
import numpy as np
import pytest

import replay_prio_ref as pr
from replay_ref import OutOfOrder

OD, NU = 3, 2


def fill(ring, steps, rng):
    """`steps` fabricated transitions per env; an episode of an env ends with probability 0.3."""
    N = ring.N
    if ring.state == pr.EMPTY:
        ring.commit(rng.standard_normal((N, OD)).astype(np.float32))
    for _ in range(steps):
        f = lambda *s: rng.standard_normal(s).astype(np.float32)
        ring.record(f(N, NU), f(N, OD), f(N), rng.random(N) < 0.2, f(N, 3), f(N, 3))
        ring.commit(f(N, OD), rng.random(N) < 0.3)


def all_cells(ring):
    slot, e = np.divmod(np.arange(ring.T * ring.N), ring.N)
    return np.stack([e, slot, np.zeros_like(e), np.zeros_like(e)], axis=1)


def test_cell_frequencies_follow_the_priorities():
    """200 draws of 256 from 300 cells whose priorities spread over four decades.  Pearson's statistic over the cells, those with an
    expected count below 5 pooled into one, against its mean plus four standard deviations under independent draws, dof + 4 sqrt(2 dof);
    stratified draws only scatter less than independent ones."""
    rng = np.random.default_rng(20)
    ring = pr.PrioRing(30, 10, OD, NU, 0.05, seed=77, p_min=1e-4, p_max=1.0, max_batch=300)
    fill(ring, 10, rng)
    prio = (10.0 ** rng.uniform(-4, 0, 300)).astype(np.float32)
    ring.update(ring.pushed, all_cells(ring), prio)
    assert np.array_equal(ring.leaves.reshape(-1), prio) and prio.max() / prio.min() > 1e3
    draws, batch = 200, 256
    counts = np.zeros(300)
    for d in range(draws):
        e, j, *_, prob = ring.prio_indices(d, batch, 0.5)
        slot = ring.slot(j)
        np.add.at(counts, slot * ring.N + e, 1)
        assert np.array_equal(prob, (ring.leaves[slot, e].astype(np.float64) / ring.total).astype(np.float32))
    expect = draws * batch * prio.astype(np.float64) / ring.total
    small = expect < 5
    obs = np.append(counts[~small], counts[small].sum())
    exp = np.append(expect[~small], expect[small].sum())
    chi2, dof = float(((obs - exp) ** 2 / exp).sum()), len(obs) - 1
    print(f"chi2 {chi2:.1f}, dof {dof}, bound {dof + 4 * np.sqrt(2 * dof):.1f}, pooled cells {int(small.sum())}")
    assert small.sum() > 0 and dof > 100                     # both kinds of cell occur: pooled rare ones and counted frequent ones
    assert chi2 < dof + 4 * np.sqrt(2 * dof)


def test_descent_ends_on_a_positive_leaf_for_every_target():
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 63, 64, 65, 300, 490, 4690):
        leaves = np.where(rng.random(n) < 0.3, 10.0 ** rng.uniform(-30, 30, n), 0).astype(np.float32)
        leaves[rng.integers(n)] = 1.0
        levels = pr.build_tree(leaves)
        total = levels[-1][0]
        u = np.concatenate([[0.0, total, np.nextafter(total, 0), np.nextafter(total, np.inf), 2 * total], rng.random(500) * total])
        got = pr.descend(levels, u)
        assert got.max() < n and np.all(leaves[got] > 0), n
    # uniform leaves: the leaf is floor(u) exactly
    levels = pr.build_tree(np.ones(490, np.float32))
    u = rng.random(1000) * 490
    assert levels[-1][0] == 490.0 and np.array_equal(pr.descend(levels, u), np.floor(u).astype(np.int64))


def test_only_stored_cells_are_drawn_and_new_ones_enter_with_p_new():
    rng = np.random.default_rng(5)
    ring = pr.PrioRing(70, 7, OD, NU, 0.05, seed=1, max_batch=256)
    with pytest.raises(OutOfOrder):
        ring.commit(np.zeros((70, OD), np.float32)) or ring.prio_indices(0, 8, 0.5)
    fill(ring, 3, rng)
    assert ring.total == 3 * 70 and np.all(ring.leaves[:3] == 1) and not ring.leaves[3:].any()
    e, j, *_ = ring.prio_indices(0, 193, 0.5)
    assert ring.slot(j).max() < 3 and j.max() < 3
    ring.update(ring.pushed, np.array([[4, 1, 0, 0]]), np.array([5.0], np.float32))
    assert ring.p_new == np.float32(5) and ring.leaves[1, 4] == np.float32(5)
    fill(ring, 5, rng)                                         # wraps: slot 0 is written again
    assert np.all(ring.leaves[0] == np.float32(5)) and np.all(ring.leaves[3] == np.float32(5)) and ring.leaves[1, 5] == 1
    with pytest.raises(OutOfOrder):
        ring.prio_indices(0, 257, 0.5)
    ring.clear()
    assert not ring.leaves.any() and ring.p_new == np.float32(1)


def test_update_clamps_skips_and_does_not_depend_on_the_order_of_rows():
    rng = np.random.default_rng(6)
    ring = pr.PrioRing(5, 4, OD, NU, 0.05, p_init=1.0, p_min=0.5, p_max=8.0, max_batch=64)
    fill(ring, 3, rng)                                         # slots 0..2 hold records 0..2; slot 3 is empty
    token = ring.pushed
    index = np.array([[0, 0], [0, 0], [1, 0], [2, 1], [3, 1], [4, 1], [0, 2], [0, 3], [5, 0], [-1, 0], [0, 4], [0, -1], [1, 2], [1, 2]])
    index = np.concatenate([index, np.zeros_like(index)], axis=1)
    prio = np.array([2.0, 3.0, np.nan, -1.0, 0.0, 1e38, 0.75, 4.0, 4.0, 4.0, 4.0, 4.0, 6.0, 0.1], np.float32)
    before = ring.leaves.copy()
    other = pr.PrioRing(5, 4, OD, NU, 0.05, p_init=1.0, p_min=0.5, p_max=8.0, max_batch=64)
    fill(other, 3, np.random.default_rng(6))
    ring.update(token, index, prio)
    other.update(token, index[::-1], prio[::-1])
    assert np.array_equal(ring.leaves, other.leaves) and ring.p_new == other.p_new == np.float32(8)
    want = before.copy()
    want[0, 0], want[0, 1], want[1, 2], want[1, 3], want[1, 4], want[2, 0], want[2, 1] = 3.0, 8.0, 0.5, 0.5, 8.0, 0.75, 6.0
    assert np.array_equal(ring.leaves, want) and not ring.leaves[3].any()
    # stale tokens: one record later slot 3 holds record 3, which a sample at `token` = 3 has not seen; T records later nothing it saw is left
    fill(ring, 1, rng)
    kept = ring.leaves.copy()
    ring.update(token, np.array([[0, 3, 0, 0]]), np.array([7.0], np.float32))
    assert np.array_equal(ring.leaves, kept)
    ring.update(token, np.array([[0, 2, 0, 0]]), np.array([7.0], np.float32))
    assert ring.leaves[2, 0] == np.float32(7)
    fill(ring, 4, rng)
    kept = ring.leaves.copy()
    ring.update(token, all_cells(ring), np.full(20, 2.5, np.float32))
    assert np.array_equal(ring.leaves, kept)
    with pytest.raises(OutOfOrder):
        ring.update(ring.pushed + 1, all_cells(ring), np.full(20, 2.5, np.float32))
    # a pending record counts as written: its cells are newer than every token
    ring.record(*[np.zeros(s, np.float32) for s in ((5, NU), (5, OD), (5,), (5,), (5, 3), (5, 3))])
    kept = ring.leaves.copy()
    ring.update(ring.pushed, np.array([[0, ring.pushed % ring.T, 0, 0]]), np.array([2.5], np.float32))
    assert np.array_equal(ring.leaves, kept)
