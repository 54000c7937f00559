"""Inputs, fp64 references, fp32 restatements and bounds for the solver's lane-group primitives (csrc/solve_g.h, solve_mf.h, devmath.h) as
tools/micro/lane_groups.hip runs them.  Plain numpy, nothing of the harness: for every family
  (a) the fp64 reference (a residual or a value formed in double precision from the fp32 inputs as stored),
  (b) a straightforward fp32 restatement of the same algorithm - sequential numpy float32, no lane tricks; a fused multiply-add is the
      double-precision expression rounded once - which only the CPU test runs, to show that the bounds can be met,
  (c) the bound, in units of u = 2^-24 times the "abs-evaluation" (the same formula with every term replaced by its absolute value).
tests/test_gpu_lane_groups.py feeds the device's outputs to the check_* functions, tests/test_lane_group_ref.py feeds the restatements'."""
import sys
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

U = 2.0 ** -24
F32 = np.float32
MAGIC = 0x5052474C
TOC = np.dtype([("name", "S32"), ("off", "<u8"), ("words", "<u8")])
LD, CW, GW, CONE_IN, CONE_OUT = 32, 36, 80, 24, 32
SENTINEL = 0xDEADBEEF
HARNESS = ROOT / "tools" / "micro" / "lane_groups.hip"


# ------------------------------------------------------------------------------------------------ the file format
def write_file(path, arrays):
    """arrays: {name: float32 / int32 / uint32 array}; flat little-endian words behind a table of contents."""
    names = list(arrays)
    assert all(len(n) < 32 for n in names), [n for n in names if len(n) >= 32]
    toc = np.zeros(len(names), TOC)
    off = 8 + toc.nbytes
    blobs = []
    for k, n in enumerate(names):
        a = np.ascontiguousarray(arrays[n])
        assert a.dtype in (np.float32, np.int32, np.uint32), (n, a.dtype)
        toc[k] = (n.encode(), off, a.size)
        off += 4 * a.size
        blobs.append(a.astype(a.dtype.newbyteorder("<")).tobytes())
    with open(path, "wb") as f:
        f.write(np.array([MAGIC, len(names)], "<i4").tobytes()); f.write(toc.tobytes())
        for b in blobs:
            f.write(b)


def read_file(path):
    raw = Path(path).read_bytes()
    magic, n = np.frombuffer(raw, "<i4", 2)
    assert magic == MAGIC
    toc = np.frombuffer(raw, TOC, n, 8)
    return {t["name"].decode(): np.frombuffer(raw, "<u4", int(t["words"]), int(t["off"])) for t in toc}


def as_f32(w): return w.view(np.float32)
def as_i32(w): return w.view(np.int32)


def fma32(a, b, c):
    """float32 fma: the double-precision product of two floats is exact, the sum is rounded to double and then to float"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


# ------------------------------------------------------------------------------------------------ A: group reductions and exchanges
GSUM6_LANES = (0, 8, 4, 12, 2, 10)
def gsum6_index(c): return ((c >> 3) & 1) + 2 * ((c >> 2) & 1) + 4 * ((c >> 1) & 1)


# the record k_groups of the harness writes per lane (GW words; 0xdeadbeef in the words nobody writes and in every word of a lane group that sat out)
GROUP_WORDS = {0: "gsum(f0)", 1: "gsum2(f0, f1).a", 2: "gsum2(f0, f1).b", 3: "gsum3(f0, f1, f2).a", 4: "gsum3.b", 5: "gsum3.c", 6: "gsum6_packed(f0..f5, c)",
               7: "gscan_incl(i0)", 8: "gor(i1)", 9: "gmax(i2)", 10: "glast(i0)", 11: "wave_or_groups(active ? i3 : 0)", 12: "wave_max_groups(active ? i3 : 0)",
               16: "16 + L: gbcast<G, L>(f3), L < G", 16 + LD: "48 + L: gbcast_after_asm<G, L>(f4), L < G"}


def group_inputs(nblocks=8, seed=11):
    """f[n, 6] floats over 1e-3 .. 1e3 with mixed signs (the first 32 lanes cancel exactly in both group sizes, the next 32 are zero),
    i[n, 4] ints: scan operand, OR operand, max operand (negative values, both extremes), a group-uniform value for the wave-level pair."""
    rng = np.random.default_rng(seed)
    n = 64 * nblocks
    f = (rng.choice([-1.0, 1.0], (n, 6)) * 10.0 ** rng.uniform(-3, 3, (n, 6))).astype(F32)
    f[8:16] = -f[0:8]; f[24:32] = -f[16:24]                # lanes 0..15 and 16..31: every value with its negative
    f[32:64] = 0
    iv = np.zeros((n, 4), np.int32)
    iv[:, 0] = rng.integers(-1000, 100000, n)
    iv[:, 1] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.int32) & rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.int32)
    iv[:, 2] = rng.integers(-2 ** 31, 2 ** 31, n)
    iv[64:96, 2] = rng.integers(-2 ** 31, -2 ** 30, 32)    # all negative
    iv[96:128, 2] = np.iinfo(np.int32).min                 # the lower extreme alone ...
    iv[128 + 5, 2] = np.iinfo(np.int32).max; iv[128 + 21, 2] = np.iinfo(np.int32).max          # ... and the upper one, in each DPP row
    iv[160:192, 2] = np.iinfo(np.int32).min; iv[160 + 30, 2] = np.iinfo(np.int32).min + 1
    gval = rng.integers(-2 ** 20, 2 ** 20, n // 32)
    gval[8:12] = -rng.integers(1, 2 ** 20, 4)              # blocks 4, 5: all negative
    iv[:, 3] = np.repeat(gval, 32)                         # uniform over 32 lanes: group-uniform for both group sizes
    return f, iv


def sum32_butterfly(v, G):
    """fp32 restatement of a group sum: v[..., G] -> the sum in every lane (rotate-and-add inside rows of 16, then the two rows)"""
    v = np.asarray(v, F32).reshape(v.shape[:-1] + (G // 16, 16))
    for k in (8, 4, 2, 1):
        v = (v + np.roll(v, k, axis=-1)).astype(F32)
    if G == 32:
        v = np.broadcast_to((v[..., 0:1, :] + v[..., 1:2, :]).astype(F32), v.shape)
    return v.reshape(v.shape[:-2] + (G,))


def restate_groups(f, iv, G, half):
    """what a faithful fp32 / int32 implementation returns, in the harness's record layout"""
    n = len(f)
    out = np.full((n, GW), SENTINEL, np.uint32)
    fg = f.reshape(-1, G, 6); ig = iv.reshape(-1, G, 4)
    rec = out.reshape(-1, G, GW)
    s = [sum32_butterfly(fg[:, :, q], G) for q in range(6)]
    for w, q in enumerate((0, 0, 1, 0, 1, 2)):
        rec[:, :, w] = s[q].view(np.uint32)
    rec[:, :, 6] = np.stack([s[min(gsum6_index(c % 16), 5)][:, c] for c in range(G)], 1).view(np.uint32)
    rec[:, :, 7] = np.cumsum(ig[:, :, 0], axis=1, dtype=np.int32).view(np.uint32)
    rec[:, :, 8] = np.broadcast_to(np.bitwise_or.reduce(ig[:, :, 1], axis=1)[:, None], (len(ig), G)).view(np.uint32)
    rec[:, :, 9] = np.broadcast_to(ig[:, :, 2].max(axis=1)[:, None], (len(ig), G)).view(np.uint32)
    rec[:, :, 10] = np.broadcast_to(ig[:, -1:, 0], (len(ig), G)).view(np.uint32)
    off = group_off(n, G, half)
    wv = np.where(off, 0, iv[:, 3]).reshape(-1, 64)[:, ::G]
    out[:, 11] = np.repeat(np.bitwise_or.reduce(wv, axis=1), 64).view(np.uint32)
    out[:, 12] = np.repeat(wv.max(axis=1), 64).view(np.uint32)
    for L in range(G):
        rec[:, :, 16 + L] = fg[:, L:L + 1, 3].view(np.uint32)
        rec[:, :, 16 + LD + L] = fg[:, L:L + 1, 4].view(np.uint32)
    out[off] = SENTINEL
    return out


def group_off(n, G, half):
    lane = np.arange(n) % 64
    return ((lane // G) & 1).astype(bool) if half else np.zeros(n, bool)


def check_groups(out, f, iv, G, half):
    """out: uint32 [n, GW].  Returns the worst |sum - ref| / (u sum|v|) seen, as a multiple of the bound (log2 G + 1)."""
    n = len(f)
    out = out.reshape(n, GW)
    off = group_off(n, G, half)
    assert (out[off] == SENTINEL).all(), "a lane group that sat out wrote something"
    live = ~off
    want = restate_groups(f, iv, G, half)
    # exact: scan, or, max, last, the wave-level pair, every broadcast, and the words nobody writes
    exact = [7, 8, 9, 10, 11, 12, 13, 14, 15] + list(range(16, GW))
    names = {7: "gscan_incl", 8: "gor", 9: "gmax", 10: "glast", 11: "wave_or_groups", 12: "wave_max_groups"}
    for w in exact:
        bad = np.flatnonzero(live & (out[:, w] != want[:, w]))
        what = names.get(w) or ("unused word" if w < 16 else "gbcast<%d>" % (w - 16) if w < 16 + LD else "gbcast_after_asm<%d>" % (w - 16 - LD))
        assert bad.size == 0, f"G={G} half={half}: {what} wrong in lanes {bad[:8]}: {out[bad[:4], w]} != {want[bad[:4], w]}"
    fo = out.view(np.float32).reshape(-1, G, GW); lv = live.reshape(-1, G)[:, 0]
    f64 = f.astype(np.float64).reshape(-1, G, 6)
    ref = f64.sum(axis=1); mag = np.abs(f64).sum(axis=1)
    bound = (np.log2(G) + 1) * U * mag
    worst = 0.0
    for w, q, name in ((0, 0, "gsum"), (1, 0, "gsum2.a"), (2, 1, "gsum2.b"), (3, 0, "gsum3.a"), (4, 1, "gsum3.b"), (5, 2, "gsum3.c")):
        s = fo[:, :, w]
        assert (s[lv].view(np.uint32) == s[lv, :1].view(np.uint32)).all(), f"G={G} half={half}: {name} differs between the lanes of a group"
        err = np.abs(s[:, 0].astype(np.float64) - ref[:, q])
        assert (err[lv] <= bound[lv, q]).all(), f"G={G} half={half}: {name} off by {np.max(err[lv] / np.maximum(bound[lv, q], 1e-300)):.2f} bounds"
        worst = max(worst, float(np.max(np.where(mag[lv, q] > 0, err[lv] / np.maximum(bound[lv, q], 1e-300), 0))))
    for c in GSUM6_LANES:
        q = gsum6_index(c)
        err = np.abs(fo[:, c, 6].astype(np.float64) - ref[:, q])
        assert (err[lv] <= bound[lv, q]).all(), f"G={G} half={half}: gsum6_packed lane {c} (sum {q}) off by {np.max(err[lv] / np.maximum(bound[lv, q], 1e-300)):.3g} bounds"
        worst = max(worst, float(np.max(np.where(mag[lv, q] > 0, err[lv] / np.maximum(bound[lv, q], 1e-300), 0))))
    return worst


# ------------------------------------------------------------------------------------------------ B: factorisations and solves
def spd_scaled(rng, n, count, dense):
    """D (B B^T + I) D with column scales over 1e-3 .. 1e3; columns >= dense keep only their diagonal entry"""
    B = rng.uniform(-1, 1, (count, n, n)); d = 10.0 ** rng.uniform(-3, 3, (count, n))
    A = (B @ B.transpose(0, 2, 1) + np.eye(n)) * d[:, :, None] * d[:, None, :]
    return tail_zeroed(A, dense), (rng.uniform(-1, 1, (count, n)) * d)


def tail_zeroed(A, dense):
    A = A.copy()
    n = A.shape[-1]
    keep = np.zeros((n, n), bool); keep[:dense, :dense] = True; keep[np.diag_indices(n)] = True
    A[:, ~keep] = 0
    return A


def hessian_like(rng, n, count, dense):
    """M + J^T W J: M as above, J of rank < dense acting on the dense block (rows repeated), W over 1 .. 1e6"""
    M, b = spd_scaled(rng, n, count, dense)
    d = np.sqrt(M[:, np.arange(n), np.arange(n)])
    r = max(dense // 2, 1)
    J = np.zeros((count, 2 * r, n))
    J[:, :r, :dense] = rng.normal(0, 0.03, (count, r, dense))
    J[:, r:] = J[:, :r] * rng.uniform(0.5, 2, (count, r, 1))                # rank r, 2 r rows
    J *= d[:, None, :]
    W = 10.0 ** rng.uniform(0, 6, (count, 2 * r))
    return M + J.transpose(0, 2, 1) @ (W[:, :, None] * J), b


def exact_cases(rng, n, count=8):
    A = np.zeros((count, n, n))
    A[0] = np.eye(n)
    for k in range(1, count):
        A[k][np.diag_indices(n)] = 4.0 ** rng.integers(-8, 9, n)               # exact roots
    return A, rng.integers(-8, 9, (count, n)).astype(np.float64)


def inertia_family(cfg, rng, count, damped):
    """M(q) (or M + h D) of a committed configuration from the fp64 mass matrix of hsr_env_amd/model.py, at random configurations"""
    from hsr_env_amd.model import load_config, mass_matrix
    m = load_config(cfg)
    qa, _ = m.scalar_joints()
    out = np.zeros((count, m.nv, m.nv))
    for k in range(count):
        q = np.array(m.qpos0, np.float64)
        q[qa] += rng.uniform(-0.5, 0.5, len(qa))
        for a in m.free_joint_qadrs():
            q[a:a + 3] += rng.uniform(-0.3, 0.3, 3)
            w = rng.normal(size=4); q[a + 3:a + 7] = w / np.linalg.norm(w)
        out[k] = mass_matrix(m, q)
        if damped:
            out[k] += m.timestep * np.diag(np.asarray(m.dof_damping, np.float64))
    scale = np.sqrt(out[:, np.arange(m.nv), np.arange(m.nv)])
    return out, rng.uniform(-1, 1, (count, m.nv)) * scale * scale


def merged_family(rng, count, nd=7, nb=3):
    """robot (nd dofs) + nb free bodies of six dofs: env k couples the robot to none, the first, the second or the third body (k % 4 - 1),
    so the envs that share a wave couple different bodies; no body couples to another"""
    n = nd + 6 * nb
    A = np.zeros((count, n, n)); b = np.zeros((count, n))
    for k in range(count):
        cb = k % 4 - 1
        idx = list(range(nd)) + (list(range(nd + 6 * cb, nd + 6 * cb + 6)) if cb >= 0 else [])
        S, bs = hessian_like(rng, len(idx), 1, len(idx))
        A[k][np.ix_(idx, idx)] = S[0]; b[k, idx] = bs[0]
        for bb in range(nb):
            if bb != cb:
                sl = slice(nd + 6 * bb, nd + 6 * bb + 6)
                S, bs = spd_scaled(rng, 6, 1, 6)
                A[k][sl, sl] = S[0]; b[k, sl] = bs[0]
    return A, b


@dataclass
class CholJob:
    kern: str; tag: str; G: int; NK: int; mode: int; nv: int; ndense: int; merged: int = 0
    A: np.ndarray = None; b: np.ndarray = None; ok: np.ndarray = None; fam: list = field(default_factory=list); padb: np.ndarray = None
    @property
    def name(self): return f"{self.kern}@{self.tag}"
    @property
    def nd_tail(self): return int(self.kern.split("_")[3]) if self.mode in (1, 3) else None

    def arrays(self):
        """the harness's view: every lane's whole row, padding as solve_body.inc pads (identity row, b = 0, diag = 1)"""
        nm, n, G = len(self.A), self.nv, self.G
        A = np.zeros((nm, G, LD), F32); A[:, np.arange(G), np.arange(G)] = 1
        A[:, :n, :n] = self.A
        b = np.zeros((nm, G), F32); b[:, :n] = self.b
        if self.padb is not None:
            b[:, n:] = self.padb
        d = np.ones((nm, G), F32); d[:, :n] = self.A[:, np.arange(n), np.arange(n)]
        return {f"{self.name}#A": A, f"{self.name}#b": b, f"{self.name}#d": d, f"{self.name}#prm": np.array([self.nv, self.ndense, self.merged], np.int32)}


def failing(base, b, dense, n, per_wave, extra=()):
    """bad matrices, each followed by per_wave - 1 sound ones: a non-positive pivot in the first, a middle and the last column (of the dense
    block and of the tail), a pivot below 1e-15, a NaN entry.  Returns (A, b, ok)."""
    mats, oks = [], []
    def add(M):
        mats.append(M); oks.append(False)
        for _ in range(per_wave - 1):
            mats.append(base.copy()); oks.append(True)
    cols = sorted({0, max(dense, 1) // 2, max(dense, 1) - 1, n - 1, min((dense + n) // 2, n - 1)} | set(extra))
    for q in cols:
        M = base.copy(); M[q, q] = -M[q, q]; add(M)
    M = base.copy(); M[n - 1, n - 1] = 0.0; add(M)
    M = np.diag(np.diag(base)).copy(); M[n // 2, n // 2] = 1e-16; add(M)
    M = base.copy(); q = max(dense, 1) // 2; M[q, q] = np.nan; add(M)
    if dense >= 2:
        M = base.copy(); M[dense - 1, 0] = M[0, dense - 1] = np.nan; add(M)
    while len(mats) % 4:
        mats.append(base.copy()); oks.append(True)
    A = np.array(mats)
    return A, np.tile(b, (len(A), 1)), np.array(oks)


def chol_jobs(seed=5):
    """every launch of section B: the product's instantiations (kPersistInstances) x routine x run-time parameters, each with all families"""
    rng = np.random.default_rng(seed)
    spec = [   # kern, G, NK, mode, [(nv, ndense)], inertia cfg
        ("fwd_16_2", 16, 2, 0, [(2, 2)], None), ("tail_16_2_0", 16, 2, 1, [(2, 0)], "cfg1"),
        ("fwd_16_8", 16, 8, 0, [(8, 8)], None), ("tail_16_8_0", 16, 8, 1, [(8, 0)], "cfg2"),
        ("fwd_16_13", 16, 13, 0, [(13, 13)], "cfg3"), ("tail_16_13_7", 16, 13, 1, [(13, 7)], "cfg3"),
        ("gen_16_13", 16, 13, 2, [(13, 0), (13, 7), (13, 13)], "cfg3"),
        ("fwd_16_16", 16, 16, 0, [(1, 1), (11, 11), (15, 15), (16, 16)], None), ("gen_16_16", 16, 16, 2, [(1, 1), (11, 11), (15, 15), (16, 16)], None),
        ("fwd_32_25", 32, 25, 0, [(25, 25)], "cfg4"), ("tail_32_25_7", 32, 25, 1, [(25, 7)], "cfg4"),
        ("fwd_32_32", 32, 32, 0, [(16, 16), (17, 17), (23, 23), (32, 32)], None),
        ("gen_32_32", 32, 32, 2, [(16, 7), (16, 16), (17, 7), (17, 17), (23, 7), (23, 23), (32, 7), (32, 32)], None),
    ]
    jobs = []
    for kern, G, NK, mode, params, cfg in spec:
        for nv, nden in params:
            dense = min(nden, nv)
            fams = [("scaled", *spd_scaled(rng, nv, 64, dense))]
            if dense >= 2:
                fams.append(("hessian", *hessian_like(rng, nv, 64, dense)))
            fams.append(("exact", *exact_cases(rng, nv)))
            if cfg is not None:
                for damped in (False, True):
                    Mi, bi = inertia_family(cfg, rng, 32, damped)
                    assert Mi.shape[1] == nv
                    keep = np.zeros((nv, nv), bool); keep[:dense, :dense] = True; keep[np.diag_indices(nv)] = True
                    if mode != 0:
                        rest = np.abs(Mi[:, ~keep]).max() if (~keep).any() else 0.0
                        if dense >= int(load_ndense(cfg)):
                            assert rest <= 1e-9, (cfg, rest)      # the tail of the real inertia matrix IS diagonal: nothing is cut off
                        Mi = tail_zeroed(Mi, dense)
                    fams.append(("inertia+hD" if damped else "inertia", Mi, bi))
            A = np.concatenate([f[1] for f in fams]).astype(F32); b = np.concatenate([f[2] for f in fams]).astype(F32)
            ok = np.ones(len(A), bool)
            fam = [(f[0], len(f[1])) for f in fams]
            if nv >= 2:
                fA, fb_, fok = failing(A[1].astype(np.float64), b[1].astype(np.float64), dense, nv, 64 // G)
                A = np.concatenate([A, fA.astype(F32)]); b = np.concatenate([b, fb_.astype(F32)]); ok = np.concatenate([ok, fok]); fam.append(("failing", len(fA)))
            jobs.append(CholJob(kern, f"n{nv}d{nden}", G, NK, mode, nv, nden, 0, A, b, ok, fam))
    # the sparse factorisation of the 32-lane instance with three free bodies: merged arm on matrices with its structure, one-by-one arm on those and on dense ones
    Am, bm = merged_family(rng, 64)
    base = Am[1]                                                       # robot coupled to body 0
    fA, fb_, fok = failing(base, bm[1], 7, 25, 2, extra=(7 + 6 + 3,))   # ... and a bad pivot inside another body
    Af = np.concatenate([Am, fA]).astype(F32); bf = np.concatenate([bm, fb_]).astype(F32); okf = np.concatenate([np.ones(64, bool), fok])
    jobs.append(CholJob("sparse_32_25_7", "merged", 32, 25, 3, 25, 25, 1, Af, bf, okf, [("merged", 64), ("failing", len(fA))]))
    Ad, bd = spd_scaled(rng, 25, 64, 25); Ah, bh = hessian_like(rng, 25, 64, 25)
    Ao = np.concatenate([Am, Ad, Ah, fA]).astype(F32); bo = np.concatenate([bm, bd, bh, fb_]).astype(F32)
    jobs.append(CholJob("sparse_32_25_7", "onebyone", 32, 25, 3, 25, 25, 0, Ao, bo, np.concatenate([np.ones(192, bool), fok]),
                        [("merged", 64), ("scaled", 64), ("hessian", 64), ("failing", len(fA))]))
    # twins with something else in the pad lanes' right-hand sides: lanes < nv must not notice
    twins = []
    for j in jobs:
        if j.name in ("fwd_16_13@n13d13", "tail_16_13_7@n13d7", "gen_16_16@n11d11", "fwd_32_32@n17d17", "gen_32_32@n23d7", "tail_32_25_7@n25d7", "sparse_32_25_7@merged", "fwd_16_2@n2d2"):
            nm = 64
            twins.append(CholJob(j.kern, j.tag + "p", j.G, j.NK, j.mode, j.nv, j.ndense, j.merged, j.A[:nm], j.b[:nm], j.ok[:nm], [("padtwin", nm)],
                                 padb=(rng.normal(0, 1e3, (nm, j.G - j.nv))).astype(F32)))
    return jobs + twins


def load_ndense(cfg):
    from hsr_env_amd.model import load_config
    return load_config(cfg).arrays["sizes"][13]


def restate_chol(job):
    """fp32 restatement: right-looking Cholesky with reciprocal roots, forward substitution folded in, column-oriented back substitution.
    Returns the harness's record [nmat, G, CW] as float32 (the pivot check as 1.0 / 0.0)."""
    nm, n, G = len(job.A), job.nv, job.G
    dense = min(job.ndense, n) if job.mode in (1, 2) else n
    L = job.A.astype(F32).copy(); b = job.b.astype(F32)
    invd = np.ones((nm, n), F32); y = np.zeros((nm, n), F32); sacc = b.copy()
    with np.errstate(all="ignore"):
        for j in range(n):
            tail_lane = job.mode == 1 and j >= dense
            inv = (1.0 / np.sqrt(L[:, j, j].astype(np.float64))).astype(F32)
            invd[:, j] = inv
            if not tail_lane:
                L[:, j:, j] = (L[:, j:, j] * inv[:, None]).astype(F32)
            y[:, j] = (sacc[:, j] * inv).astype(F32)
            if j < dense:
                l = L[:, j + 1:, j]
                L[:, j + 1:, j + 1:] = fma32(-l[:, :, None], l[:, None, :], L[:, j + 1:, j + 1:])
            sacc[:, j + 1:] = fma32(-L[:, j + 1:, j], y[:, j:j + 1], sacc[:, j + 1:])
        x = np.zeros((nm, n), F32)
        for j in range(n - 1, -1, -1):
            if job.mode == 1 and j >= dense:
                x[:, j] = ((b[:, j] * invd[:, j]).astype(F32) * invd[:, j]).astype(F32)
                continue
            acc = np.zeros(nm, F32)
            for i in range(j + 1, n):
                acc = (acc - (L[:, i, j] * x[:, i]).astype(F32)).astype(F32)
            x[:, j] = ((y[:, j] + acc).astype(F32) * invd[:, j]).astype(F32)
    rec = np.zeros((nm, G, CW), F32)
    rec[:, np.arange(G), np.arange(G)] = 1
    rec[:, :n, :n] = np.tril(L)
    rec[:, :n, LD] = invd; rec[:, n:, LD] = 1; rec[:, :n, LD + 1] = y; rec[:, :n, LD + 2] = x
    good = (invd > 0) & (invd < 3.2e7)
    rec[:, :, LD + 3] = good.all(axis=1)[:, None]
    return rec


def check_chol(job, rec, require_y=None):
    """rec: float32 [nmat, G, CW] (word LD + 3 as an integer in the device's record: pass ok separately through rec_ok).  Asserts the
    bounds of the module docstring for every matrix that factors and the pivot verdicts for all; returns the worst ratios to the bounds."""
    nm, n, G = len(job.A), job.nv, job.G
    rec = rec.reshape(nm, G, CW)
    okw = rec[:, :, LD + 3].view(np.uint32) != 0
    want = job.ok
    assert (okw == want[:, None]).all(), f"{job.name}: pivot check wrong for matrices {np.flatnonzero((okw != want[:, None]).any(axis=1))[:8]} (families {job.fam})"
    g = np.flatnonzero(want)
    A = job.A[g].astype(np.float64); b = job.b[g].astype(np.float64)
    L = np.tril(rec[g][:, :n, :n].astype(np.float64)); invd = rec[g][:, :n, LD].astype(np.float64)
    y = rec[g][:, :n, LD + 1].astype(np.float64); x = rec[g][:, :n, LD + 2].astype(np.float64)
    assert np.isfinite(rec[g][:, :n, LD:LD + 3]).all() and np.isfinite(L).all(), f"{job.name}: non-finite result for a matrix that factors"
    di = np.arange(n)
    if job.mode == 1:          # a tail lane keeps its pivot as invd only: L[c][c] = 1 / invd there
        nd = job.ndense
        L[:, di[nd:], di[nd:]] = 1.0 / invd[:, nd:]
    tri = np.tril(np.ones((n, n), bool))
    aL = np.abs(L); LLt = aL @ aL.transpose(0, 2, 1)
    worst = {}
    def ratio(name, err, bound):
        if err.size == 0:
            return
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))
        k = np.unravel_index(np.argmax(r), r.shape)
        assert r[k] <= 1.0, f"{job.name}: {name} is {r[k]:.3g} x its bound at matrix {g[k[0]]} {k[1:]} (families {job.fam})"
        worst[name] = float(r[k])
    ratio("|A - L L^T|", np.abs(A - L @ L.transpose(0, 2, 1))[:, tri], ((n + 8) * U * LLt)[:, tri])
    if job.mode != 1:
        ratio("|invd L_cc - 1|", np.abs(invd * L[:, di, di] - 1), np.full((len(g), n), 6 * U))
    else:
        ratio("|invd L_cc - 1|", np.abs(invd[:, :job.ndense] * L[:, di[:job.ndense], di[:job.ndense]] - 1), np.full((len(g), job.ndense), 6 * U))
    if job.mode in (0, 3) if require_y is None else require_y:
        ratio("|L y - b|", np.abs((L @ y[:, :, None])[:, :, 0] - b), (n + 4) * U * ((aL @ np.abs(y)[:, :, None])[:, :, 0] + np.abs(b)))
    ratio("|A x - b|", np.abs((A @ x[:, :, None])[:, :, 0] - b), (3 * n + 8) * U * ((LLt @ np.abs(x)[:, :, None])[:, :, 0] + np.abs(b)))
    return worst


# ------------------------------------------------------------------------------------------------ C: the MFMA accumulators
HESS_KERNELS = (("hess16_13", 16, 13), ("hess16_16", 16, 16), ("hess32_25", 32, 25), ("hess32_32", 32, 32))
HESS_R = (1, 5, 48)
HESS_BIG = 1e15


def hess_inputs(seed=3, nblk=4):
    """{job: (A[nblk, R, 64], B, row0[nblk, 64, 32], R)}: different operands per block and lane; in block 1 the second env's operands are a
    large constant (nothing of it may reach another env)"""
    rng = np.random.default_rng(seed)
    jobs = {}
    for kern, G, NK in HESS_KERNELS:
        for R in HESS_R:
            A = (rng.choice([-1.0, 1.0], (nblk, R, 64)) * 10.0 ** rng.uniform(-3, 3, (nblk, R, 64))).astype(F32)
            B = (rng.choice([-1.0, 1.0], (nblk, R, 64)) * 10.0 ** rng.uniform(-3, 3, (nblk, R, 64))).astype(F32)
            A[1, :, G:2 * G] = HESS_BIG; B[1, :, G:2 * G] = HESS_BIG
            r0 = (rng.normal(0, 10, (nblk, 64, LD))).astype(F32)
            jobs[f"{kern}@r{R}"] = (A, B, r0, R)
    return jobs


def hess_arrays(jobs):
    out = {}
    for name, (A, B, r0, R) in jobs.items():
        out[name + "#A"] = A; out[name + "#B"] = B; out[name + "#r0"] = r0; out[name + "#prm"] = np.array([R], np.int32)
    return out


def _hess_terms(A, B, G):
    nblk, R, _ = A.shape
    a = A.astype(np.float64).reshape(nblk, R, 64 // G, G); bb = B.astype(np.float64).reshape(nblk, R, 64 // G, G)
    return a, bb


def restate_hess(A, B, r0, G, NK):
    a, bb = _hess_terms(A, B, G)
    nblk, R = A.shape[:2]
    acc = np.zeros((nblk, 64 // G, G, G), F32)          # [block, env, lane c, register k]
    for r in range(R):
        acc = fma32(a[:, r, :, None, :], bb[:, r, :, :, None], acc)
    out = r0.copy().reshape(nblk, 64 // G, G, LD)
    out[..., :NK] = (out[..., :NK] + acc[..., :NK]).astype(F32)
    out[..., G:] = 0          # (the record has no registers >= G)
    return out.reshape(nblk, 64, LD)


def check_hess(out, A, B, r0, G, NK):
    nblk, R = A.shape[:2]
    a, bb = _hess_terms(A, B, G)
    out = out.reshape(nblk, 64 // G, G, LD).astype(np.float64); r0 = r0.reshape(nblk, 64 // G, G, LD).astype(np.float64)
    ref = r0.copy(); mag = np.abs(r0)
    ref[..., :G] += np.einsum("nrek,nrec->neck", a, bb); mag[..., :G] += np.einsum("nrek,nrec->neck", np.abs(a), np.abs(bb))
    ref[..., NK:G] = r0[..., NK:G]; ref[..., G:] = 0          # registers >= NK are not touched (the record has none >= G)
    err = np.abs(out - ref); bound = (R + 1) * U * mag
    assert (err[..., NK:] == 0).all(), "add_rows wrote a register >= NK"
    r = err[..., :NK] / bound[..., :NK]
    k = np.unravel_index(np.argmax(r), r.shape)
    assert r[k] <= 1.0, f"G={G} NK={NK} R={R}: block {k[0]} env {k[1]} lane {k[2]} register {k[3]}: {out[k]:.9g}, want {ref[k]:.9g} ({r[k]:.3g} bounds)"
    return float(r[k])


# ------------------------------------------------------------------------------------------------ D: the elliptic cone
CONE_MU = (1e-3, 0.1, 1.0, 2.0)
CONE_DIMS = (1, 3, 4, 6)


def _cone_pack(mu, fri, D, x, v):
    p = np.zeros(CONE_IN, F32)
    dim = len(x)
    p[0] = mu; p[1:dim] = fri[:dim - 1]; p[6:6 + dim] = D; p[12:12 + dim] = x; p[18:18 + dim] = v
    return p


def cone_inputs(seed=7, per_zone=256):
    """float32 [n, 24] (mu, fri[5], D[6], x[6], v[6]; rows >= dim zero as the callers pad) and per point (dim, kind): kind 0 a random point
    of a zone (drawn well inside it), 1 the T sweep, 2 T = 0, 3 a point placed exactly on a zone boundary, 4 T > 0 with T^2 below the smallest normal float.  D[j] = D[0] fri[j-1]^2 / mu^2
    for the friction rows, the relation of the model under which cost and gradient are continuous across the lower boundary."""
    rng = np.random.default_rng(seed)
    pts, meta = [], []
    def add(dim, mu, fri, D0, x, kind):
        D = np.concatenate([[D0], D0 * fri[:dim - 1] ** 2 / mu ** 2])
        v = rng.normal(size=dim) * 10.0 ** rng.uniform(-2, 1)
        pts.append(_cone_pack(mu, fri, D, x, v)); meta.append((dim, kind))
    for dim in CONE_DIMS:
        for mu in CONE_MU:
            for zone in (0, 1, 2):
                if dim == 1 and zone == 2:
                    continue
                for _ in range(per_zone):
                    fri = 10.0 ** rng.uniform(-3, 0, 5); D0 = 10.0 ** rng.uniform(0, 6)
                    x = rng.normal(size=dim) * 10.0 ** rng.uniform(-4, 1)
                    if dim > 1:
                        # from the values as the device will see them, so that the margin to the boundary is what is drawn here
                        T = float(np.sqrt(np.sum((x[1:].astype(F32).astype(np.float64) * fri[:dim - 1].astype(F32).astype(np.float64)) ** 2)))
                        s = rng.uniform(0.02, 3)
                        N = {0: mu * T * (1 + s), 1: -T / mu * (1 + s), 2: T * (-1 / mu + (mu + 1 / mu) * rng.uniform(0.02, 0.98))}[zone]
                        x[0] = N / mu
                    else:
                        x[0] = abs(x[0]) if zone == 0 else -abs(x[0])
                    add(dim, mu, fri, D0, x, 0)
    for dim in (3, 6):                                   # T from 1 down to where T^2 leaves the float range, inside the middle zone (N = 0)
        for mu in CONE_MU:
            for D0 in (1.0, 1e6):
                for e in np.arange(0, -18.51, -0.5):          # T^2 = 1.25e-37 at the end: the last half-decade above the smallest normal float
                    x = np.zeros(dim); x[1] = 10.0 ** e; x[2] = 0.5 * 10.0 ** e
                    add(dim, mu, np.array([1.0, 0.5, 0.25, 0.125, 1.0]), D0, x, 1)
    for dim in (3, 4, 6):                                # T = 0: above, at and below the apex
        for mu in CONE_MU:
            for x0 in (0.3, 0.0, -0.3):
                x = np.zeros(dim); x[0] = x0
                add(dim, mu, 10.0 ** rng.uniform(-3, 0, 5), 100.0, x, 2)
    for dim in (3, 4, 6):                                # exactly on the boundaries: T = 5 exactly, N = mu T and mu N + T = 0 exactly, and one ulp to either side
        for mu, x_top, x_bot in ((1.0, 5.0, -5.0), (2.0, 5.0, -1.25)):
            for x0 in (x_top, x_bot):
                for step in (0, 1, -1):
                    x = np.zeros(dim); x[1] = 3.0; x[2] = 4.0
                    x[0] = np.nextafter(F32(x0), F32(np.inf if step > 0 else -np.inf)) if step else x0
                    add(dim, mu, np.ones(5), 64.0, x, 3)
    for dim in (3, 6):                                   # T > 0 whose T^2 is subnormal in float (or gone): only "finite" and the zone can be asked, see cone_ratios
        for mu in CONE_MU:
            for D0 in (1.0, 1e6):
                for e in (-19.5, -20.5, -21.5, -22.4):
                    for x0 in (0.0, -1e-21):
                        x = np.zeros(dim); x[0] = x0; x[1] = 10.0 ** e
                        add(dim, mu, np.array([1.0, 0.5, 0.25, 0.125, 1.0]), D0, x, 4)
    while len(pts) % 64:
        add(1, 1.0, np.ones(5), 1.0, np.array([1.0]), 2)
    return np.array(pts, F32), np.array(meta, np.int32)


def cone_zone64(mu, fri, x):
    """zones of many points at once in fp64 (the conditions of Problem.cone): arrays [n], [n, 5], [n, 6]"""
    N = mu * x[:, 0]
    T = np.sqrt(np.sum((x[:, 1:] * fri) ** 2, axis=1))
    top = (N >= mu * T) | ((T <= 0) & (N >= 0))
    bot = ~top & ((mu * N + T <= 0) | ((T <= 0) & (N < 0)))
    return np.where(top, 0, np.where(bot, 1, 2))


def cone_reference(pin, meta):
    """fp64 values (Problem.cone of tests/test_oracle_optimality.py, checked there by finite differences) on the inputs as stored, the
    abs-evaluations that scale the bounds, and which points keep their zone when every coordinate moves by +-4 ulp."""
    from test_oracle_optimality import Problem
    n = len(pin)
    p = pin.astype(np.float64)
    mu, fri, D, x, v = p[:, 0], p[:, 1:6], p[:, 6:12], p[:, 12:18], p[:, 18:24]
    zone = cone_zone64(mu, fri, x)
    ulp = np.spacing(np.abs(pin[:, 12:18])).astype(np.float64)
    stable = np.ones(n, bool)
    moves = [s * 4 * ulp * (np.arange(6) == j) for j in range(6) for s in (1, -1)]
    out_dir = np.where(x >= 0, 1.0, -1.0); out_dir[:, 0] = -1.0            # tangential rows outwards, normal row down - and the reverse
    moves += [4 * ulp * out_dir, -4 * ulp * out_dir]
    for mv in moves:
        stable &= cone_zone64(mu, fri, x + mv) == zone
    ref = dict(zone=zone, stable=stable, cost=np.zeros(n), g=np.zeros((n, 6)), H=np.zeros((n, 6, 6)), d1=np.zeros(n), d2=np.zeros(n),
               cost_abs=np.zeros(n), g_abs=np.zeros((n, 6)), H_abs=np.zeros((n, 6, 6)))
    for i in range(n):
        dim = int(meta[i, 0])
        c, g, H = Problem.cone(x[i, :dim], D[i, :dim], mu[i], fri[i], True)
        ref["cost"][i] = c; ref["g"][i, :dim] = g; ref["H"][i, :dim, :dim] = H
    # abs-evaluations per zone formula
    aN = np.abs(mu * x[:, 0]); Uj = np.abs(x[:, 1:] * fri); T = np.sqrt(np.sum(Uj ** 2, axis=1))
    bot_cost = 0.5 * np.sum(D * x * x, axis=1); bot_g = np.abs(D * x); bot_H = np.zeros((n, 6, 6)); bot_H[:, np.arange(6), np.arange(6)] = D
    Dm = D[:, 0] / (mu * mu * (1 + mu * mu)); NTa = aN + mu * T
    with np.errstate(all="ignore"):
        dNT = np.concatenate([mu[:, None], mu[:, None] * Uj * fri / T[:, None]], axis=1)
        dNT[~np.isfinite(dNT)] = 0
        mid_cost = 0.5 * Dm * NTa ** 2; mid_g = (Dm * NTa)[:, None] * dNT
        mid_H = Dm[:, None, None] * dNT[:, :, None] * dNT[:, None, :]
        core = (np.eye(5)[None] / T[:, None, None] + Uj[:, :, None] * Uj[:, None, :] / T[:, None, None] ** 3) * fri[:, :, None] * fri[:, None, :]
        core[~np.isfinite(core)] = 0
        mid_H[:, 1:, 1:] += (Dm * NTa * mu)[:, None, None] * core
    for key, b_, m_ in (("cost_abs", bot_cost, mid_cost), ("g_abs", bot_g, mid_g), ("H_abs", bot_H, mid_H)):
        own = np.where((zone == 1).reshape((-1,) + (1,) * (b_.ndim - 1)), b_, np.where((zone == 2).reshape((-1,) + (1,) * (b_.ndim - 1)), m_, 0 * b_))
        # a point whose zone is not settled may be evaluated by either neighbour's formula: cost and gradient are continuous, each formula's rounding is bounded by its own abs-evaluation
        ref[key] = np.where(stable.reshape((-1,) + (1,) * (b_.ndim - 1)), own, np.maximum(b_, m_))
    ref["d1"] = np.einsum("nj,nj->n", ref["g"], v); ref["d1_abs"] = np.einsum("nj,nj->n", ref["g_abs"], np.abs(v))
    ref["d2"] = np.einsum("nj,njk,nk->n", v, ref["H"], v); ref["d2_abs"] = np.einsum("nj,njk,nk->n", np.abs(v), ref["H_abs"], np.abs(v))
    return ref


def restate_cone(pin):
    """fp32 restatement of cone_eval2 / cone_cost / cone_dd, vectorised over the points: the harness's record as uint32 [n, 32]"""
    n = len(pin)
    mu, fri, D, x, v = pin[:, 0], pin[:, 1:6], pin[:, 6:12], pin[:, 12:18], pin[:, 18:24]
    f = lambda a: np.asarray(a, F32)
    rcp = lambda a: f(1.0 / a.astype(np.float64))
    with np.errstate(all="ignore"):
        Uv = f(x[:, 1:] * fri); Nn = f(x[:, 0] * mu)
        T2 = np.zeros(n, F32); S1 = np.zeros(n, F32); S2 = np.zeros(n, F32)
        fv = f(fri * v[:, 1:])
        for j in range(5):
            T2 = fma32(Uv[:, j], Uv[:, j], T2); S1 = fma32(Uv[:, j], fv[:, j], S1); S2 = fma32(fv[:, j], fv[:, j], S2)
        T = f(np.sqrt(T2.astype(np.float64)))
        top = (Nn >= f(mu * T)) | ((T <= 0) & (Nn >= 0))
        bot = ~top & ((fma32(mu, Nn, T) <= 0) | ((T <= 0) & (Nn < 0)))
        mid = ~top & ~bot
        zone = np.where(top, 0, np.where(bot, 1, 2))
        out = np.zeros((n, CONE_OUT), F32)
        # bottom
        cb = np.zeros(n, F32); d1b = np.zeros(n, F32); d2b = np.zeros(n, F32)
        for j in range(6):
            cb = fma32(f(f(0.5 * D[:, j]) * x[:, j]), x[:, j], cb); d1b = fma32(f(D[:, j] * x[:, j]), v[:, j], d1b); d2b = fma32(f(D[:, j] * v[:, j]), v[:, j], d2b)
        # middle
        Dm = f(D[:, 0] * rcp(f(f(mu * mu) * f(1 + f(mu * mu))))); NT = fma32(-mu, T, Nn); invT = rcp(T)
        kappa = f(f(-Dm * NT) * mu)
        ki = f(kappa * invT)
        k3, sc = cone_k3(ki, T2)
        us = f(f(fri * Uv) * sc[:, None])
        gn = np.zeros((n, 6), F32); gn[:, 0] = mu
        gn[:, 1:] = f(f(f(-mu[:, None] * Uv) * fri) * invT[:, None])
        dw = np.zeros((n, 6), F32); dw[:, 1:] = f(f(f(kappa[:, None] * fri) * fri) * invT[:, None])
        gm = f(f(Dm * NT)[:, None] * gn); cm = f(f(f(0.5 * Dm) * NT) * NT)
        gnv = f(mu * fma32(-invT, S1, v[:, 0]))
        d1m = f(f(Dm * NT) * gnv)
        S1s = f(S1 * sc)
        d2m = f(fma32(f(Dm * gnv), gnv, f(ki * S2)) - f(f(k3 * S1s) * S1s))
        out[:, 0] = np.where(mid, cm, np.where(bot, cb, 0)); out[:, 1] = np.where(mid, Dm, 0); out[:, 2] = np.where(mid, k3, 0)
        out[:, 4:10] = np.where(mid[:, None], gm, np.where(bot[:, None], f(D * x), 0))
        out[:, 10:16] = np.where(mid[:, None], dw, np.where(bot[:, None], D, 0))
        out[:, 16:22] = np.where(mid[:, None], gn, 0)
        out[:, 22:28] = 0; out[:, 23:28] = np.where(mid[:, None], us, 0)
        out[:, 28] = out[:, 0]; out[:, 29] = np.where(mid, d1m, np.where(bot, d1b, 0)); out[:, 30] = np.where(mid, d2m, np.where(bot, d2b, 0))
    w = out.view(np.uint32).copy()
    w[:, 3] = zone; w[:, 31] = 0
    return w


def cone_k3(ki, T2):
    """(k3, scale) of the middle zone's -k3 u u^T term as cone_eval2 / cone_dd form it: k3 = (kappa / T) / T^2 and scale = 1, or - below T^2 = 2^-64, where
    k3 alone leaves the float range long before the product does - (k3 2^-80, 2^40): u, or S1 of cone_dd, is multiplied by the scale, the product is the same"""
    tiny = T2 < F32(2.0 ** -64)
    k3 = (ki * (1.0 / (T2 * np.where(tiny, F32(2.0 ** 80), F32(1))).astype(np.float64)).astype(F32)).astype(F32)
    return k3, np.where(tiny, F32(2.0 ** 40), F32(1)).astype(F32)


def cone_ratios(w, pin, meta, ref):
    """w: the record uint32 [n, 32].  Asserts what needs no K (finite outputs, zones, which points may be left out of the Hessian comparison)
    and returns the worst error of each quantity in units of u x abs-evaluation, over all points and over the settled ones."""
    n = len(pin)
    w = w.reshape(n, CONE_OUT)
    o = w.view(np.float32).astype(np.float64)
    fl = np.delete(w.view(np.float32), 3, axis=1)
    bad = np.flatnonzero(~np.isfinite(fl).all(axis=1))
    assert bad.size == 0, f"non-finite cone output at points {bad[:8]} (kind {meta[bad[:8], 1]}): x = {pin[bad[0], 12:18]}, mu = {pin[bad[0], 0]}, record {fl[bad[0]]}"
    zone = w[:, 3].view(np.int32)
    st = ref["stable"]
    placed = (meta[:, 1] == 3) | ((meta[:, 1] == 2) & (pin[:, 12] == 0))          # on a boundary on purpose: kind 3, and the apex x = 0 where all three zones meet
    assert st[~placed].all(), "a point that was not placed on a boundary is left out of the Hessian comparison"
    # kind 4: T^2 is subnormal or zero in float while T > 0.  T has lost its bits (or is 0 where the hardware's square root flushes its operand), so no K u bound
    # can hold; what holds is that every output is finite (above) and that the zone is the fp64 one or the one T = 0 gives
    sub = meta[:, 1] == 4
    judged = ~sub
    zone_t0 = np.where(pin[:, 0].astype(np.float64) * pin[:, 12] >= 0, 0, 1)
    assert ((zone == ref["zone"]) | (zone == zone_t0))[sub].all(), f"zone of a point with subnormal T^2 is neither the fp64 one nor that of T = 0: {np.flatnonzero(sub & (zone != ref['zone']) & (zone != zone_t0))[:8]}"
    st = st & judged
    assert (zone[st] == ref["zone"][st]).all(), f"zone differs at settled points {np.flatnonzero(st & (zone != ref['zone']))[:8]}"
    v = pin[:, 18:24].astype(np.float64)
    g, dw, gn, uu = o[:, 4:10], o[:, 10:16], o[:, 16:22], o[:, 22:28]
    H = o[:, 1, None, None] * gn[:, :, None] * gn[:, None, :] - o[:, 2, None, None] * uu[:, :, None] * uu[:, None, :]
    H[:, np.arange(6), np.arange(6)] += dw
    def rat(err, mag, where=judged):
        r = np.where(mag > 0, err / np.where(mag > 0, mag, 1) / U, np.where(err > 0, np.inf, 0.0))
        r = r.reshape(n, -1).max(axis=1)
        return float(r[where].max())
    return {
        "cost": rat(np.abs(o[:, 0] - ref["cost"]), ref["cost_abs"]), "cone_cost": rat(np.abs(o[:, 28] - ref["cost"]), ref["cost_abs"]),
        "g": rat(np.abs(g - ref["g"]), ref["g_abs"]), "d1": rat(np.abs(o[:, 29] - ref["d1"]), ref["d1_abs"]),
        "H": rat(np.abs(H - ref["H"]), ref["H_abs"], st), "d2": rat(np.abs(o[:, 30] - ref["d2"]), ref["d2_abs"], st),
    }


# K of section D: four times the worst ratio of the fp32 restatement above against fp64 on cone_inputs(), and not below 16
# (tests/test_lane_group_ref.py measures the ratio again and asserts that this constant is what the rule gives for it)
CONE_RESTATEMENT_WORST = 7.914          # u x abs-evaluation, in the assembled Hessian (cost 5.39, g 5.94, d1 4.61, d2 4.34)
CONE_K = max(16.0, 4 * CONE_RESTATEMENT_WORST)          # 31.66


# ------------------------------------------------------------------------------------------------ E: fast_sincos
def sincos_inputs(seed=1):
    rng = np.random.default_rng(seed)
    x = [rng.uniform(-20, 20, 200000)]
    for k in range(-26, 27):                             # every multiple of pi / 4 up to |x| = 20
        if abs(k * np.pi / 4) <= 20:
            x.append(k * np.pi / 4 + np.linspace(-1e-3, 1e-3, 101))
    x.append(np.array([0.0, -0.0, 1e-30, -1e-30, 20.0, -20.0]))
    x = np.concatenate(x).astype(F32)
    x = x[np.abs(x) <= 20]
    pad = (-len(x)) % 64
    return np.concatenate([x, np.zeros(pad, F32)])


def restate_sincos(x):
    f = lambda a: np.asarray(a, F32)
    k = np.rint(f(x * F32(0.63661977236758134)))
    r = fma32(k, F32(-1.5703125), x); r = fma32(k, F32(-4.837512969970703125e-4), r); r = fma32(k, F32(-7.54978995489188e-8), r)
    z = f(r * r)
    ps = fma32(f(fma32(fma32(F32(-1.9515295891e-4), z, F32(8.3321608736e-3)), z, F32(-1.6666654611e-1)) * z), r, r)
    pc = fma32(fma32(fma32(F32(2.443315711809948e-5), z, F32(-1.388731625493765e-3)), z, F32(4.166664568298827e-2)), f(z * z), fma32(F32(-0.5), z, F32(1.0)))
    q = k.astype(np.int64) & 3
    s0 = np.where(q & 1, pc, ps); c0 = np.where(q & 1, ps, pc)
    return np.stack([np.where(q & 2, -s0, s0), np.where((q + 1) & 2, -c0, c0)], axis=1).astype(F32)


def check_sincos(out, x):
    out = out.reshape(-1, 2).astype(np.float64); x64 = x.astype(np.float64)
    es = np.abs(out[:, 0] - np.sin(x64)).max(); ec = np.abs(out[:, 1] - np.cos(x64)).max()
    en = np.abs(out[:, 0] ** 2 + out[:, 1] ** 2 - 1).max()
    assert es <= 2.0 ** -23 and ec <= 2.0 ** -23, f"|s - sin x| <= {es:.3g}, |c - cos x| <= {ec:.3g}: above 2^-23 = {2.0 ** -23:.3g}"
    assert en <= 4 * U, f"|s^2 + c^2 - 1| <= {en:.3g}: above 4 u = {4 * U:.3g}"
    return {"sin": es / 2.0 ** -23, "cos": ec / 2.0 ** -23, "norm": en / (4 * U)}


# ------------------------------------------------------------------------------------------------ everything, once
_CACHE = {}


def all_inputs():
    """every array of the input file and the descriptions the checks need; built once per process"""
    if not _CACHE:
        gf, gi = group_inputs()
        cj = chol_jobs()
        hj = hess_inputs()
        cp, cm = cone_inputs()
        sx = sincos_inputs()
        arrays = {}
        for kern in ("grp16", "grp16h", "grp32", "grp32h"):
            arrays[f"{kern}@a#f"] = gf; arrays[f"{kern}@a#i"] = gi
        for j in cj:
            arrays.update(j.arrays())
        arrays.update(hess_arrays(hj))
        arrays["cone@a#in"] = cp; arrays["sincos@a#x"] = sx
        _CACHE.update(arrays=arrays, groups=(gf, gi), chol=cj, hess=hj, cone=(cp, cm), sincos=sx)
    return _CACHE
