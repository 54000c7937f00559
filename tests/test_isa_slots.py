"""Issue slots of the solver's dependent DPP chains, read from the device assembly (no GPU needed; tools/isa_slots.py does the counting).

1. gfx9 wants two issue slots between a VALU write of a VGPR and a DPP read of it.  The compiler pads what it emits itself; it cannot see
   into an asm string.  tests/test_isa_hazards.py checks the hand-written DPP instructions against producers that are hand-written
   themselves; since the pivot steps of the 16-lane factorisations became single asm statements without pads (csrc/solve_g.h,
   chol_step16 / chol_step16_fwd: the two slots are filled with the step's own work), the guard is widened to ANY producer: in the cfg3 and
   cfg4 instances no hand-written DPP instruction reads, as its DPP source, a register written fewer than two issue slots earlier
   (an `s_nop N` counts N + 1 slots).

2. The wait states of the cfg3 Newton window (first v_mfma to 1500 instructions past the last: two Hessians, two factorisations, back
   substitution, line search, evaluation) are at most 300.  Derivation: the window had 426.  Each of its two copies of chol_g_fwd paid
   nine wait states in every one of its 13 pivot steps; taking the nine out of the nine steps that have at least four trailing updates
   (enough independent work to fill every distance) is 2 x 9 x 9 = 162, which leaves 264; the paired group sums of the back substitution
   and the line search take more, and 300 leaves room for the compiler's own placement of what is left.  Measured after the change: 253 (kernel 1197 -> 988)."""
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HIPCC = "/opt/rocm/bin/hipcc"
sys.path.insert(0, str(ROOT / "tools"))
import isa_slots  # noqa: E402

NEWTON_WAIT_STATES_MAX = 300


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    """The device assembly of every kernel instance, compiled once for the module with the product build's flags."""
    out = tmp_path_factory.mktemp("isa") / "hsrsim.s"
    sys.path.insert(0, str(ROOT))
    from hsr_env_amd.build import CODEGEN_FLAGS
    subprocess.check_call([HIPCC, *CODEGEN_FLAGS, "-S", "--cuda-device-only", "-Wno-unused-result", "-Wno-unused-value",
                           "-o", str(out), str(ROOT / "hsr_env_amd" / "csrc" / "hsrsim.hip")], stderr=subprocess.DEVNULL)
    return out.read_text()


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not available")
def test_no_hand_written_dpp_read_within_two_slots_of_a_write(assembly):
    names = re.findall(r"^(_Z13k_env_step_mf\w*DevModel_cfg[34]Lb[01]E\w+):", assembly, flags=re.M)
    assert len(names) == 4, names          # cfg3 plain / with the solo-server path, cfg4 with its pair tables in LDS / in global memory
    for name in names:
        _, ins = isa_slots.kernel_body(assembly, name)
        hand = [d for _, d, _, h in isa_slots.dpp_distances(ins) if h]
        assert len(hand) > 100, (name, "the hand-written DPP instructions were not found in the assembly")
        fewest, close = isa_slots.min_hand_written_distance(ins)
        print(name, "hand-written DPP instructions:", len(hand), "fewest slots since the write of a DPP source:", fewest)
        assert not close, (name, close[:3])


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not available")
def test_wait_states_of_the_cfg3_newton_window(assembly):
    name, ins = isa_slots.kernel_body(assembly, "DevModel_cfg3Lb0E")
    lo, hi = isa_slots.newton_window(ins, 1500)
    n, nops, ws = isa_slots.counts(ins[lo:hi])
    print(name, "newton window:", n, "instructions,", nops, "s_nop,", ws, "wait states")
    assert n > 2000, (name, lo, hi)          # the window was found: the Hessian's matrix-core instructions and what follows them
    assert ws <= NEWTON_WAIT_STATES_MAX, (nops, ws)
