"""The solver's lane-group primitives against fp64 references of the same operations: the DPP group sums / scans / broadcasts, the in-register
Cholesky factorisations and triangular solves, the MFMA Hessian accumulators, the three elliptic-cone functions (csrc/solve_g.h, solve_mf.h)
and fast_sincos (csrc/devmath.h).  tools/micro/lane_groups.hip calls the product routines on the inputs of tests/lane_group_ref.py - compiled
once, run once, by the module's fixture; every test below only reads the arrays that run left behind and judges them with the bounds of
lane_group_ref (Higham's componentwise bounds for Cholesky and its solves, (log2 G + 1) u for a tree sum, (R + 1) u for R accumulated
products, K u for the cone with K from the fp32 restatement's own error, 2^-23 for sin / cos): conditioning does not enter any of them, so a
result outside is a finding.  tests/test_gpu_dpp_chains.py pins the bits of the same routines; this module pins their mathematics."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import lane_group_ref as ref

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def outs(tmp_path_factory):
    """one compile, one device run: {array name: uint32 words}.  A failure here fails every test of the module without running anything again."""
    d = tmp_path_factory.mktemp("lane_groups")
    exe, fin, fout = d / "lane_groups", d / "in.bin", d / "out.bin"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-o", str(exe), str(ref.HARNESS)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    print("lane_groups: compiled once")
    ref.write_file(fin, ref.all_inputs()["arrays"])
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=60)
    print(r.stdout.strip() or "lane_groups: no output", "(one device run)")
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    return ref.read_file(fout)


@pytest.mark.parametrize("G,half", [(16, False), (16, True), (32, False), (32, True)])
def test_group_reductions_and_exchanges(outs, G, half):
    """gsum / gsum2 / gsum3 bit-equal in every lane of a group and within (log2 G + 1) u sum|v| of the fp64 sum (exact cancellation and all-zero
    groups included); gsum6_packed in its six destination lanes, over both DPP rows for G = 32; gscan_incl, gor, gmax, glast, every gbcast and
    gbcast_after_asm lane and the wave-level OR / max exact; lane groups that sat out behind a group-uniform branch keep their sentinel.
    NOT covered: wave_or_groups / wave_max_groups called under a partial EXEC mask.  Their contract forbids it (v_readlane ignores EXEC: wave-uniform code only, value
    defined in every lane), and the harness calls them as solve_body.inc does - whole wave active, the groups that sit out contributing `active ? x : 0`."""
    f, iv = ref.all_inputs()["groups"]
    worst = ref.check_groups(outs[f"grp{G}{'h' if half else ''}@a#out"], f, iv, G, half)
    print(f"G={G} half={half}: worst group sum error = {worst:.3f} of its bound")


def _chol(outs, modes, twins=False):
    seen = 0
    for job in ref.all_inputs()["chol"]:
        if job.mode not in modes or job.tag.endswith("p") != twins:
            continue
        rec = outs[job.name + "#out"].view(np.float32).reshape(len(job.A), job.G, ref.CW)
        worst = ref.check_chol(job, rec)
        print(f"{job.name:28s} nv={job.nv:2d} ndense={job.ndense:2d} {len(job.A):3d} matrices: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        seen += 1
    assert seen


def test_chol_g_fwd_and_back_substitution(outs):
    """chol_g_fwd + chol_back_mf, every instantiation and run-time nv: A = L L^T, invd, L y = b and A x = b within Higham's bounds; failed pivots seen by
    the whole group and by no other group of the wave."""
    _chol(outs, (0,))


def test_chol_g_tail_and_its_solve(outs):
    """chol_g_tail + chol_solve_tail (ND = 0 and 7): a tail lane's pivot is its invd; M and M + h D of the committed configurations among the inputs.
    chol_solve_tail does not hand out y: judged by |A - L L^T|, invd and |A x - b| only (|L y - b| is asserted where y exists: chol_g_fwd, chol_sparse_fwd)."""
    _chol(outs, (1,))


def test_chol_g_and_chol_solve_mf(outs):
    """chol_g + chol_solve_mf with run-time nv and ndense (ndense < nv: the block-diagonal tail at run time).  chol_solve_mf does not hand out y: judged by
    |A - L L^T|, invd and |A x - b| only."""
    _chol(outs, (2,))


def test_sparse_factorisation_both_arms(outs):
    """chol_sparse_fwd + chol_sparse_back<32, 25, 7>: the merged arm on robot + one coupled body (a different body in neighbouring envs), the one-by-one arm
    on those and on dense matrices; a bad body pivot fails its env alone."""
    _chol(outs, (3,))


def test_pad_lanes_do_not_reach_the_result(outs):
    """the same matrices with other right-hand sides in the lanes >= nv: rows, invd, y, x and the verdict of the lanes < nv are equal bit for bit"""
    jobs = {j.name: j for j in ref.all_inputs()["chol"]}
    seen = 0
    for name, tw in jobs.items():
        if not tw.tag.endswith("p"):
            continue
        base = jobs[name[:-1]]
        nm, n = len(tw.A), tw.nv
        a = outs[base.name + "#out"].reshape(len(base.A), base.G, ref.CW)[:nm, :n]
        b = outs[tw.name + "#out"].reshape(nm, tw.G, ref.CW)[:, :n]
        keep = np.zeros((n, ref.CW), bool); keep[:, ref.LD:] = True; keep[:, :n] = np.tril(np.ones((n, n), bool))
        diff = np.argwhere((a != b) & keep)
        assert diff.size == 0, f"{name}: (matrix, lane, word) {diff[:6].tolist()} depend on the pad lanes' right-hand side"
        ref.check_chol(tw, outs[tw.name + "#out"].view(np.float32).reshape(nm, tw.G, ref.CW))
        seen += 1
    assert seen >= 6


def test_hessian_accumulators(outs):
    """HessAcc::add_rows<13|16> and HessAcc32::add_rows<25|32> after R = 1, 5, 48 rank-1 MFMA terms: lane c, register k = row0[k] + sum_r A_r[k] B_r[c] of its own env
    within (R + 1) u abs-evaluation; one env's operands are 1e15 and nothing of them reaches a neighbour; registers >= NK untouched."""
    for kern, G, NK in ref.HESS_KERNELS:
        for R in ref.HESS_R:
            A, B, r0, _ = ref.all_inputs()["hess"][f"{kern}@r{R}"]
            worst = ref.check_hess(outs[f"{kern}@r{R}#out"].view(np.float32), A, B, r0, G, NK)
            print(f"{kern} R={R:2d}: worst error = {worst:.3f} of its bound")


def test_cone_functions(outs):
    """cone_eval2, cone_cost, cone_dd on 256 random points per (dim, mu, zone), the T sweep down to the underflow of T^2, T = 0 and points exactly on the zone
    boundaries.  Everywhere: finite outputs; cost, g, cone_cost, d1 within K u abs-evaluation of fp64.  Where the fp64 zone survives +-4 ulp in every
    coordinate (all but the points placed on a boundary): equal zone, H = diag(dw) + Dm gn gn^T - k3 u u^T within K u abs-evaluation, d2 = v^T H v.
    Points with T > 0 whose T^2 is subnormal in float: finite outputs, and the fp64 zone or the zone of T = 0 - T has no bits left for a K u bound there.
    K = max(16, 4 x worst ratio of the fp32 restatement against fp64 on these inputs) = 4 x 7.914 = 31.66 (lane_group_ref.CONE_RESTATEMENT_WORST: the assembled Hessian;
    cost 5.39, g 5.94, d1 4.61, d2 4.34; measured again by tests/test_lane_group_ref.py)."""
    pin, meta = ref.all_inputs()["cone"]
    cref = ref.cone_reference(pin, meta)
    ratios = ref.cone_ratios(outs["cone@a#out"], pin, meta, cref)
    print("cone: worst error / (u abs-evaluation): " + ", ".join(f"{k} {v:.2f}" for k, v in ratios.items()) + f"  (K = {ref.CONE_K})")
    for k, v in ratios.items():
        assert v <= ref.CONE_K, f"{k}: {v:.3g} u abs-evaluation, K = {ref.CONE_K}"


def test_fast_sincos(outs):
    """200 000 points over |x| <= 20, clusters around every multiple of pi / 4, +-0, 1e-30: |s - sin x|, |c - cos x| <= 2^-23, |s^2 + c^2 - 1| <= 4 u"""
    x = ref.all_inputs()["sincos"]
    worst = ref.check_sincos(outs["sincos@a#out"].view(np.float32), x)
    print("fast_sincos: " + ", ".join(f"{k} {v:.3f} of its bound" for k, v in worst.items()))
