"""The solver's dependent DPP chains after their issue slots were filled (csrc/solve_g.h: chol_step16 / chol_step16_fwd, gsum2 / gsum3; csrc/solve_mf.h:
the back substitutions) against frozen copies of the routines as they were: tools/micro/dpp_chains.hip factors and solves 256 seeded SPD matrices
(column scales over 1e-3 .. 1e3, one with a non-positive pivot in the middle) with both and compares row[0..c], invd, y and x word by word - the
cfg3 instance (G = 16, NK = 13), the block-diagonal tail (ND = 7) and the 32-lane instance (NK = 25) whose broadcast runs cross lane 16 - and every
multi-sum against gsum in every lane, also with every second lane group switched off.  Only the order of issue may differ: not one bit of a result.
This module pins the BITS: a mistake that the rewritten and the frozen routine share passes here.  What the routines compute - that the factor is a
Cholesky factor and the solves solve, within Higham's bounds, for every instantiation and run-time nv / ndense - is pinned by tests/test_gpu_lane_groups.py."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.gpu
def test_chains_bit_identical_to_the_frozen_routines(tmp_path):
    exe = tmp_path / "dpp_chains"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-w", "-o", str(exe), str(ROOT / "tools" / "micro" / "dpp_chains.hip")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "mismatches: 0" in r.stdout
    assert r.stdout.count("255 of 256 factorisations pass") == 6, r.stdout          # the failed pivot is seen, every sound matrix passes
