"""cone_eval2 (csrc/solve_g.h) forms every output once, by select, instead of merging a zero-initialised struct across one early return per zone.
tools/micro/cone_merge.hip runs it against a frozen copy of the early-return form, one point per lane and 64 rows per wave, and this module
compares all 28 output fields of every row word by word: cost, Dm, k3, zone, g[6], dw[6], gn[6], u[6].  Not one bit may differ - the zeros
outside the middle zone and the scaled pair (k3 2^-80, u 2^40) below T^2 = 2^-64 included.

Rows (seeded, finite): every zone for dim 1, 3, 4 and 6 with the rows beyond dim zero-padded (D = x = fri = 0), D log-uniform over 1 .. 1e6;
T = 0 with Nn > 0, Nn = +-0 and Nn < 0; T^2 below 2^-64 in the middle zone; and sweeps of Nn over nine consecutive floats around mu T and of
mu Nn around -T for mu a power of two: the device's T is within an ulp of the exact one and mu T is exact, so the sweep steps over the boundary
between two neighbouring floats, and the first point on the far side IS Nn == mu T (mu Nn + T == 0) - asserted as the zone change inside every sweep.
The order of the rows decides which lanes share a wave: blocks of one zone (the wave-uniform skip of the middle zone taken, and not taken),
shuffled blocks, and blocks with lanes switched off behind a divergent branch.  This module pins the BITS against the previous form; what the
function computes is pinned against fp64 by tests/test_gpu_lane_groups.py."""
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
IN_W, OUT_W = 20, 28
F32 = np.float32
FIELDS = ["cost", "Dm", "k3", "zone"] + [f"{n}[{j}]" for n in ("g", "dw", "gn", "u") for j in range(6)]


def _rows(rng, n, dim, zone, tscale=None, mu=None, fmin=1e-4):
    """n rows of dimension dim aimed at a zone (0 top, 1 bottom, 2 middle), a clear margin from the boundaries; T = 0 for dim 1."""
    r = np.zeros((n, IN_W), F32)
    mu = rng.choice([0.25, 0.5, 1.0, 2.0, 0.3, 0.7, 1.3], n).astype(F32) if mu is None else np.full(n, mu, F32)
    f0, f2, f3 = (np.exp(rng.uniform(np.log(fmin), 0.0, n)).astype(F32) for _ in range(3))
    fri = np.stack([f0, f0, f2, f3, f3], 1)
    fri[:, dim - 1:] = 0
    D = np.exp(rng.uniform(0.0, np.log(1e6), (n, 6))).astype(F32)
    D[:, dim:] = 0
    scale = np.exp(rng.uniform(np.log(1e-6), np.log(1e2), n)) if tscale is None else np.exp(rng.uniform(np.log(tscale[0]), np.log(tscale[1]), n))
    x = (rng.choice([-1.0, 1.0], (n, 6)) * rng.uniform(0.2, 1.0, (n, 6)) * scale[:, None]).astype(F32)
    x[:, dim:] = 0
    T = np.sqrt(((x[:, 1:].astype(np.float64) * fri) ** 2).sum(1))
    m = mu.astype(np.float64)
    u = rng.uniform(0.05, 0.95, n)
    if zone == 0: Nn = m * T * (1 + 3 * u) + (T == 0) * u
    elif zone == 1: Nn = -(T / m) * (1 + 3 * u) - (T == 0) * u
    else: Nn = T * (-1 / m + (m + 1 / m) * u)
    x[:, 0] = (Nn / m).astype(F32)
    r[:, 0] = mu; r[:, 1:6] = fri; r[:, 6:12] = D; r[:, 12:18] = x
    return r


def _sweep(rng, mu, bottom):
    """Nine rows, Nn = x0 mu over consecutive floats centred on mu T (top boundary) or on -T / mu (bottom boundary); mu a power of two, one tangential row."""
    r = _rows(rng, 9, 3, 2, mu=mu)
    r[:] = r[0]
    r[:, 14] = 0          # x[2] = 0: T = |x[1] fri[0]|, which fp32 forms exactly up to the square root's last bit
    T = np.abs(F32(r[0, 13]) * F32(r[0, 1]))
    c = F32(-T / F32(mu) / F32(mu)) if bottom else F32(T)          # x0: Nn = x0 mu = mu T, or mu Nn = x0 mu^2 = -T
    v = c
    for _ in range(4): v = np.nextafter(v, F32(-np.inf))
    for k in range(9):
        r[k, 12] = v
        v = np.nextafter(v, F32(np.inf))
    return r


def _inputs():
    rng = np.random.default_rng(20251)
    blocks, kinds = [], []

    def add(rows, kind, shuffle=False, off=0.0):
        rows = rows.copy()
        assert len(rows) % 64 == 0
        if shuffle: rows = rows[rng.permutation(len(rows))]
        on = (rng.uniform(size=len(rows)) >= off).astype(np.uint32)
        rows.view(np.uint32)[:, 18] = on
        blocks.append(rows); kinds.extend([kind] * (len(rows) // 64))

    for dim in (1, 3, 4, 6):
        zones = (0, 1) if dim == 1 else (0, 1, 2)
        for z in zones: add(_rows(rng, 64, dim, z), f"single{z}")                                  # a wave in ONE zone
        add(np.concatenate([_rows(rng, 64, dim, z) for z in zones]), "mixed", shuffle=True)          # lanes of a wave in different zones
        add(np.concatenate([_rows(rng, 64, dim, z) for z in zones]), "mixed_off", shuffle=True, off=0.3)
    # T = 0 in a contact that has friction rows: Nn > 0, Nn < 0, Nn = +0 and -0
    t0 = np.concatenate([_rows(rng, 32, 6, 0), _rows(rng, 32, 6, 1)])
    t0[:, 13:18] = 0
    t0[:8, 12] = 0.0; t0[8:16, 12] = -0.0
    add(t0, "t0")
    # T^2 < 2^-64 (T below 2.3e-10), middle zone, down to T of the order of 1e-17; with the other zones in the same waves
    tiny = [_rows(rng, 64, dim, 2, tscale=(1e-16, 1e-10), fmin=0.05) for dim in (3, 4, 6)]          # (fmin: T^2 stays a normal number)
    add(np.concatenate(tiny + [_rows(rng, 32, 6, 0, tscale=(1e-16, 1e-10)), _rows(rng, 32, 6, 1, tscale=(1e-16, 1e-10))]), "tiny", shuffle=True)
    # the exact boundaries: 7 sweeps of 9 rows + one filler per block, mu a power of two
    sweeps = []
    for bottom in (False, True):
        rows = []
        for k in range(14):
            rows.append(_sweep(rng, [0.5, 1.0, 2.0, 0.25][k % 4], bottom))
            sweeps.append((sum(len(b) for b in blocks) + 64 * (k // 7) + 9 * (k % 7), bottom))
            if k % 7 == 6: rows.append(_rows(rng, 1, 6, 2))
        add(np.concatenate(rows), "sweep")
    # D at the ends of its range
    ends = np.concatenate([_rows(rng, 64, 6, z) for z in (0, 1, 2)])
    ends[:96, 6:12] = 1.0; ends[96:, 6:12] = 1e6
    add(ends, "ends", shuffle=True)
    data = np.concatenate(blocks)
    assert np.isfinite(data[:, :18]).all()
    return data, kinds, sweeps


@pytest.mark.gpu
def test_cone_eval2_bit_identical_to_the_early_return_form(tmp_path):
    sys.path.insert(0, str(ROOT))
    from hsr_env_amd.build import CODEGEN_FLAGS
    exe, fin, fout = tmp_path / "cone_merge", tmp_path / "in.bin", tmp_path / "out.bin"
    r = subprocess.run([HIPCC, *CODEGEN_FLAGS, "-w", "-o", str(exe), str(ROOT / "tools" / "micro" / "cone_merge.hip")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    data, kinds, sweeps = _inputs()
    n = len(data)
    data.tofile(fin)
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
    out = np.fromfile(fout, np.uint32).reshape(2, n, OUT_W)
    new, old = out[0], out[1]
    on = data.view(np.uint32)[:, 18] != 0
    zone = old[:, 3].astype(np.int64)
    # the inputs reached what they were aimed at (read off the FROZEN function's zones)
    assert (old[~on] == 0xdeadbeef).all() and (new[~on] == 0xdeadbeef).all()
    assert set(zone[on]) == {0, 1, 2}
    per_block = [set(zone[b * 64:(b + 1) * 64][on[b * 64:(b + 1) * 64]]) for b in range(n // 64)]
    assert all(per_block[b] == {int(k[-1])} for b, k in enumerate(kinds) if k.startswith("single")), "single-zone waves"
    assert sum(s == {0, 1, 2} for s in per_block) >= 6 and any(s == {0, 1} for s in per_block)          # the skip runs both ways, also in mixed waves
    t0 = [b for b, k in enumerate(kinds) if k == "t0"][0] * 64
    assert (zone[t0:t0 + 32] == 0).all() and (zone[t0 + 32:t0 + 64] == 1).all()          # T = 0: the sign of Nn decides, +-0 is top
    tb = [b for b, k in enumerate(kinds) if k == "tiny"][0] * 64
    tsl = slice(tb, tb + 256)
    T2 = ((data[tsl, 13:18].astype(np.float64) * data[tsl, 1:6]) ** 2).sum(1)
    assert ((T2 < 2.0 ** -66) & (zone[tsl] == 2)).sum() >= 100          # scaled (k3, u) pairs in the middle zone
    for start, bottom in sweeps:
        z = list(zone[start:start + 9])
        far = 1 if bottom else 0
        assert far in z and 2 in z, (start, bottom, z)          # the boundary lies between two neighbouring floats of the sweep
    # the comparison
    bad = np.argwhere(new != old)
    for i, k in bad[:10]:
        print(f"row {i} ({kinds[i // 64]}, lane {i % 64}, zone {zone[i]}) {FIELDS[k]}: {new[i, k]:#010x} != frozen {old[i, k]:#010x}   in: {data[i, :18]}")
    print(f"{n} rows, {int(on.sum())} switched on, zones {np.bincount(zone[on], minlength=3)}, mismatching words: {len(bad)}")
    assert len(bad) == 0
