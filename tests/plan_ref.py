"""Checker-side restatement of the device planner (include/hsrsim.h: hsr_plan), in numpy, written from its specification and not from the
kernels: the Irwin-Hall draw from the Philox of tests/episode_ref.py, the clamp, the cost recursion, the rank rule, the fixed tree of the
refit's sums, the refit, shift and reset.  The product never imports it.

Every float32 operation is a float32 numpy operation of its own and every fp64 operation a float64 one, so all of it is bit-exact against
the device except the one fp64 square root of the refit, whose rounding is not pinned (sigma: one float32 ulp).
"""
import numpy as np

import episode_ref as ep

STREAM_PLAN = 7
f32, f64 = np.float32, np.float64
SQRT3 = f32(1.7320508075688772)
WAVE = 64


# ------------------------------------------------------------------ the draw
def z_from_words(w):
    """uint32 [..., 4] -> float32 [...]: (((u0 + u1) + (u2 + u3)) - 2) sqrt(3), u = (w >> 8) 2^-24."""
    u = (np.asarray(w, np.uint32) >> np.uint32(8)).astype(f32) * f32(2.0 ** -24)
    a, b = (u[..., 0] + u[..., 1]).astype(f32), (u[..., 2] + u[..., 3]).astype(f32)
    return (((a + b).astype(f32) - f32(2)).astype(f32) * SQRT3).astype(f32)


def plan_words(seed, env_offset, P, K, H, nu, call, it, h):
    """The Philox blocks of step h: uint32 [P, K, nu, 4]."""
    ctr = np.zeros((P, K, nu, 4), np.uint32)
    ctr[..., 0] = ((int(env_offset) + np.arange(P, dtype=np.int64)) & ep.MASK).astype(np.uint32)[:, None, None]
    ctr[..., 1] = (int(call) * 256 + int(it)) & ep.MASK
    ctr[..., 2] = STREAM_PLAN
    k, a = np.arange(K, dtype=np.int64)[:, None], np.arange(nu, dtype=np.int64)[None, :]
    ctr[..., 3] = (((k * H + h) * nu + a) & ep.MASK).astype(np.uint32)[None]
    return ep.philox4x32_10(ctr, ep._key(seed))


def z_draws(seed, env_offset, P, K, H, nu, call, it, h):
    """float32 [P, K, nu]; candidate 0 takes z = 0."""
    z = z_from_words(plan_words(seed, env_offset, P, K, H, nu, call, it, h))
    z[:, 0, :] = 0
    return z


def ctrl_range(ctrlrange):
    """(lo, hi) float32 [nu]: a side without a limit (not finite, or the marker 1e30) counts as -1 / +1."""
    cr = np.asarray(ctrlrange, f32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        lo = np.where(np.abs(cr[:, 0]) < f32(1e30), cr[:, 0], f32(-1)).astype(f32)
        hi = np.where(np.abs(cr[:, 1]) < f32(1e30), cr[:, 1], f32(1)).astype(f32)
    return lo, hi


def half_range(lo, hi):
    return ((hi - lo).astype(f32) * f32(0.5)).astype(f32)


def clamp(x, lo, hi):
    x = np.asarray(x, f32)
    return np.where(x < lo, lo, np.where(x > hi, hi, x)).astype(f32)


def sample(mean, sigma, z, h, lo, hi):
    """mean, sigma float32 [P, H, nu], z float32 [P, K, nu] -> ctrl float32 [P, K, nu]."""
    step = (sigma[:, None, h, :] * z).astype(f32)
    return clamp((mean[:, None, h, :] + step).astype(f32), lo, hi)


def reset_state(P, H, lo, hi, init_std):
    mean = np.broadcast_to(clamp(np.zeros(len(lo), f32), lo, hi), (P, H, len(lo))).copy()
    sigma = np.broadcast_to((f32(init_std) * half_range(lo, hi)).astype(f32), (P, H, len(lo))).copy()
    return mean, sigma


def reset(mean, sigma, mask, lo, hi, init_std):
    m0, s0 = reset_state(mean.shape[0], mean.shape[1], lo, hi, init_std)
    sel = np.ones(mean.shape[0], bool) if mask is None else np.asarray(mask) != 0
    mean, sigma = mean.copy(), sigma.copy()
    mean[sel], sigma[sel] = m0[sel], s0[sel]
    return mean, sigma


def shift(mean, sigma, mask, lo, hi, init_std):
    _, s0 = reset_state(mean.shape[0], mean.shape[1], lo, hi, init_std)
    sel = np.ones(mean.shape[0], bool) if mask is None else np.asarray(mask) != 0
    mean, sigma = mean.copy(), sigma.copy()
    mean[sel] = np.concatenate([mean[sel, 1:], mean[sel, -1:]], axis=1)
    sigma[sel] = s0[sel]
    return mean, sigma


# ------------------------------------------------------------------ the cost
def dist(a, g):
    """sqrt((dx dx + dy dy) + dz dz) in float32, operation by operation."""
    d = (np.asarray(a, f32) - np.asarray(g, f32)).astype(f32)
    sq = (d * d).astype(f32)
    s = ((sq[..., 0] + sq[..., 1]).astype(f32) + sq[..., 2]).astype(f32)
    return np.sqrt(s).astype(f32)


class Costs:
    def __init__(self, n):
        self.J, self.g = np.zeros(n, f32), np.ones(n, f32)
        self.alive, self.reach = np.ones(n, bool), np.full(n, -1, np.int32)

    def step(self, d, done, bad, h, gamma):
        d, done, bad = np.asarray(d, f32), np.asarray(done) != 0, np.asarray(bad) != 0
        live = self.alive.copy()
        hit, go = live & bad, live & ~bad
        with np.errstate(invalid="ignore", over="ignore"):
            self.J = np.where(go, (self.J + (self.g * d).astype(f32)).astype(f32), self.J).astype(f32)
            self.g = np.where(go, (self.g * f32(gamma)).astype(f32), self.g).astype(f32)
        self.J[hit] = np.inf
        self.reach[go & done] = h
        self.alive = live & ~bad & ~done

    def add(self, extra):
        with np.errstate(invalid="ignore", over="ignore"):
            self.J = (self.J + np.asarray(extra, f32)).astype(f32)


# ------------------------------------------------------------------ rank, tree, refit
def cost_keys(J):
    """A NaN or an infinity of either sign counts as +inf, by the bits."""
    J = np.ascontiguousarray(J, f32)
    finite = (J.view(np.uint32) & np.uint32(0x7f800000)) != np.uint32(0x7f800000)
    return np.where(finite, J, f32(np.inf)).astype(f32), finite


def ranks(keys):
    """rank(k) = #{ j : key_j < key_k or (key_j == key_k and j < k) } for keys [K]."""
    keys = np.asarray(keys, f32)
    j, k = np.arange(len(keys))[None, :], np.arange(len(keys))[:, None]
    return ((keys[None, :] < keys[:, None]) | ((keys[None, :] == keys[:, None]) & (j < k))).sum(axis=1)


def tree_depth(K):
    return (K + WAVE - 1) // WAVE + 6


def tree_sum(leaves):
    """float64 [..., K] -> float64 [...] in the fixed shape: lane l adds the leaves l, l + 64, .. serially from 0.0, then the 64 lanes in the
    tree v[l] += v[l + off], off = 32 .. 1.  (A lane's missing leaves are padded with +0.0, which changes no bit of a sum begun at +0.0.)"""
    leaves = np.asarray(leaves, f64)
    K = leaves.shape[-1]
    rows = (K + WAVE - 1) // WAVE
    pad = np.zeros(leaves.shape[:-1] + (rows * WAVE,), f64)
    pad[..., :K] = leaves
    pad = pad.reshape(leaves.shape[:-1] + (rows, WAVE))
    v = np.zeros(leaves.shape[:-1] + (WAVE,), f64)
    for r in range(rows):
        v = v + pad[..., r, :]
    off = 32
    while off >= 1:
        v = v.copy()
        v[..., :off] = v[..., :off] + v[..., off:2 * off]
        off //= 2
    return v[..., 0]


def update(mean, sigma, act, J, elites, alpha, min_std, half):
    """One group: mean, sigma float32 [H, nu], act float32 [H, nu, K] (the actions as sampled), J float32 [K], half = half_range [nu].
    -> (mean, sigma, elite mask [K], best index, best cost, failed: 0 / 1); sigma through numpy's correctly rounded float64 sqrt."""
    keys, finite = cost_keys(J)
    r = ranks(keys)
    E = min(int(elites), int(finite.sum()))
    elite = r < E
    best = int(np.flatnonzero(r == 0)[0])
    if E == 0:
        return mean.copy(), sigma.copy(), elite, best, keys[best], 1
    x = np.asarray(act, f32).astype(f64)
    m = tree_sum(np.where(elite, x, 0.0)) / f64(E)
    d = x - m[..., None]
    v = tree_sum(np.where(elite, d * d, 0.0)) / f64(E)
    al = f64(f32(alpha))
    mu, sg = mean.astype(f64), sigma.astype(f64)
    new_mean = (mu + al * (m - mu)).astype(f32)
    snew = sg + al * (np.sqrt(v) - sg)
    floor = f64(f32(min_std)) * np.asarray(half, f32).astype(f64)
    new_sigma = np.maximum(snew, floor[None, :]).astype(f32)
    return new_mean, new_sigma, elite, best, keys[best], 0
