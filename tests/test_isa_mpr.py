"""Issue slots the convex narrowphase spends without doing arithmetic, read from the device assembly (no GPU needed; tools/isa_copies.py --lines does the counting).

The wave that sets the launch time is alone on its SIMD and issue-bound: a plain `v_mov_b32`, a wait state and a scalar instruction on the exec mask each
cost it a full slot.  Counted: plain copies + `s_nop` wait states + SALU instructions that read or write exec, over the instructions of the cfg3 instance
of k_env_step_mf whose INNERMOST source line lies in the MPR functions of csrc/collide.h - sup_merge, support_vertex, support (every inlined call site
of it) and everything from `struct Sup` to the end of mpr_penetration.  The arithmetic helpers of devmath.h they call are not in the count.

Parent (d975bc0), measured with the same tool and the same flags at that commit: 1 090 = 397 copies + 156 wait states + 537 exec-mask SALU, in 3 481 instructions.

Bound: PARENT - 108.  Derivation, per inlined `support<8>` call site - there are twelve: five mpr_support calls of mpr_penetration with two each, and the two of
the margin rescan in persist.h:
1. the three DPP exchanges of the scan's winner move two registers each; without bound_ctrl every one of the six moves was preceded by a copy that
   zeroed its destination.  With bound_ctrl they need none: 12 x 6 = 72 copies.
2. the type dispatch had four arms at every site.  cfg3's convex pairs hold boxes, cylinders and meshes as first geom and boxes and meshes as second
   (cfg_consts.h: cv_types), so the six first-geom sites lose the sphere arm and the six second-geom sites the sphere and the cylinder arm: 18 arms, each
   entered by one exec-mask instruction and left by one: 36.
What the compiler makes of the shorter dispatch beyond that (the parent's ran as a binary tree of type comparisons with two to three mask instructions per
node; the cylinder arm's wait states) is NOT in the bound: it is the compiler's room.  Nor is the third step of the change: the scan's compare lost its bound
test, four scalar ANDs per pass and site that do not touch exec and are not counted here.  Measured after the change: 888 = 308 + 151 + 429, in 3 117
instructions (kernel 19 627 -> 18 881).

The listing is that of tests/test_isa_copies.py (product CODEGEN_FLAGS plus -gline-tables-only, which changes no instruction), with -DHSR_DEV_CFG3: only the
cfg3 instance is compiled - the same template instance, a sixth of the compile time."""
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HIPCC = "/opt/rocm/bin/hipcc"
sys.path.insert(0, str(ROOT / "tools"))
import isa_copies  # noqa: E402
import isa_slots  # noqa: E402

PARENT_MPR_NO_WORK_SLOTS = 1090
MPR_NO_WORK_SLOTS_MAX = PARENT_MPR_NO_WORK_SLOTS - 12 * 6 - 18 * 2
KERNEL = "DevModel_cfg3Lb0E"


def mpr_lines():
    """[(file, first, last)] of the MPR functions in csrc/collide.h: sup_merge to the end of support, `struct Sup` to the end of mpr_penetration."""
    src = (ROOT / "hsr_env_amd" / "csrc" / "collide.h").read_text().split("\n")

    def line(pattern, after=0):
        return next(k for k, t in enumerate(src, 1) if k > after and re.search(pattern, t))
    a0 = line(r"\bvoid sup_merge\(")
    a1 = line(r"^struct ContactOut\b", a0)
    b0 = line(r"^struct Sup\b")
    b1 = line(r"^// conservative culls", b0)
    assert any("bool mpr_penetration(" in t for t in src[b0:b1]) and any(" v3 support(" in t for t in src[a0:a1])
    return [("collide.h", a0, a1 - 1), ("collide.h", b0, b1 - 1)]


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not available")
def test_slots_without_arithmetic_in_the_mpr_functions_of_the_cfg3_instance(tmp_path):
    sys.path.insert(0, str(ROOT))
    from hsr_env_amd.build import CODEGEN_FLAGS
    out = tmp_path / "hsrsim_cfg3.s"
    subprocess.check_call([HIPCC, *CODEGEN_FLAGS, "-gline-tables-only", "-DHSR_DEV_CFG3", "-S", "--cuda-device-only", "-Wno-unused-result", "-Wno-unused-value",
                           "-o", str(out), str(ROOT / "hsr_env_amd" / "csrc" / "hsrsim.hip")], stderr=subprocess.DEVNULL)
    listing = out.read_text()
    name, ins = isa_slots.kernel_body(listing, KERNEL)
    locs = isa_copies.kernel_locs(listing, KERNEL)
    assert locs is not None and len(locs) == len(ins), "the listing carries no line table"
    rows = isa_copies.line_account(ins, locs, mpr_lines())
    tot = [sum(r[k] for r in rows.values()) for k in range(len(isa_copies.ACCOUNT))]
    slots = isa_copies.no_work_slots(rows)
    print(name, "MPR functions:", dict(zip(isa_copies.ACCOUNT, tot)), "copies + wait states + exec-mask SALU:", slots, "kernel:", len(ins), "instructions")
    assert tot[0] > 2000, "the MPR functions were not found in the line table"
    assert slots <= MPR_NO_WORK_SLOTS_MAX, (slots, dict(zip(isa_copies.ACCOUNT, tot)))
