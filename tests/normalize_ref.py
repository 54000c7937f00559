"""An fp64 numpy restatement of the running-moments normaliser (include/hsrsim.h: hsr_norm), for the tests: the moments over the
concatenation of all counted rows, two-pass; the publish rule; the float32 apply.  It knows nothing of batches, merges or sum shapes - that
is the point: the device's state after any sequence of updates must agree with the state of all counted rows taken at once."""
import numpy as np

EPS, CLIP = 0.01, 5.0          # the defaults (those of the HER baselines)


def counted(rows, mask=None):
    """The rows an update counts: selected by the mask (None: all) and finite throughout.  -> (rows [m, dim] float64, rows skipped)."""
    rows = np.asarray(rows, dtype=np.float32)
    sel = np.ones(len(rows), bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    fin = np.isfinite(rows).all(axis=1)
    return rows[sel & fin].astype(np.float64), int((sel & ~fin).sum())


def moments(updates, dim):
    """updates: [(rows, mask or None), ..] -> (count, mean [dim], m2 [dim], skipped) of all counted rows together, two-pass in fp64."""
    kept, skipped = [], 0
    for rows, mask in updates:
        k, s = counted(rows, mask)
        kept.append(k.reshape(-1, dim)); skipped += s
    x = np.concatenate(kept) if kept else np.zeros((0, dim))
    if len(x) == 0:
        return 0.0, np.zeros(dim), np.zeros(dim), skipped
    mean = x.sum(axis=0) / len(x)
    m2 = ((x - mean) ** 2).sum(axis=0)
    return float(len(x)), mean, m2, skipped


def publish(count, mean, m2, eps=EPS):
    """-> (mean32, rstd32) float32 [dim]; eps is the float32 the library was given."""
    mean, m2 = np.asarray(mean, np.float64), np.asarray(m2, np.float64)
    if not count > 0:
        return np.zeros(mean.shape, np.float32), np.ones(mean.shape, np.float32)
    eps = float(np.float32(eps))
    std = np.sqrt(np.maximum(m2 / count, eps * eps))
    return mean.astype(np.float32), (1.0 / std).astype(np.float32)


def apply(x, mean32, rstd32, clip=CLIP):
    """clamp((x - mean32) rstd32, -clip, clip): two float32 operations, each rounded on its own; comparisons, so a NaN stays a NaN."""
    x, clip = np.asarray(x, dtype=np.float32), np.float32(clip)
    with np.errstate(invalid="ignore", over="ignore"):
        y = ((x - np.asarray(mean32, np.float32)).astype(np.float32) * np.asarray(rstd32, np.float32)).astype(np.float32)
        y = np.where(y > clip, clip, y)
        y = np.where(y < -clip, -clip, y)
    return y.astype(np.float32)


def merge(a, b):
    """Chan's rule for two (count, mean, m2) triples."""
    (na, ma, qa), (nb, mb, qb) = a, b
    if not nb > 0:
        return a
    delta, tot = mb - ma, na + nb
    return tot, ma + delta * nb / tot, qa + (qb + delta * delta * na * nb / tot)
