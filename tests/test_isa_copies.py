"""Issue slots the Newton iteration spends on plain register copies, read from the device assembly (no GPU needed; tools/isa_copies.py does the counting).

The wave that sets the launch time is alone on its SIMD and issue-bound: a `v_mov_b32` that only moves a value costs it as much as an FMA.  The cfg3
Newton window (first v_mfma to 1500 instructions past the last, as in tests/test_isa_slots.py: two Hessians, two factorisations, back substitution,
line search, ONE inlined cone evaluation with its stores) is held to

1. at most PARENT - 80 plain copies.  Derivation: the outputs of cone_eval2 (csrc/solve_g.h) were a struct zeroed first and filled per zone behind early
   returns, which compiled to one copy per field and arm - 74 in the window's evaluation (25 before the first test, 27 in the "not top" arm, 19 at the end
   of the bottom arm, 3 more) - and eval_at regrouped dw into the registers of its wide stores with 6 more.  Formed once, by select, in the registers
   they are stored from, they need none: 80.  What the Hessian's start could give on top of that (up to 29 per build_H copy) is NOT in the bound: it
   is the compiler's room for its own placement.  Measured with tools/isa_copies.py: parent (dd43196) 233 copies, 161 of them in 11 runs of five or
   more; after the change 151, 85 in 8 runs (kernel 1704 -> 1442).  Of the parent's 80, 61 lay inside the window - it ends inside the evaluation -, so the cone alone
   leaves 181; the literal-zero accumulator of the Hessian's first matrix-core product (2 x 16) brings the count under the bound.
2. no run of eight or more consecutive plain copies that belongs to the cone functions of solve_g.h (the parent had runs of 25 and 26 there).

The listing is compiled once for the module, with the product's CODEGEN_FLAGS plus -gline-tables-only: the `.loc` lines name the source of every
instruction and change none (the instruction streams of the listings with and without it were compared for this change: identical)."""
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

PARENT_NEWTON_COPIES = 233
NEWTON_COPIES_MAX = PARENT_NEWTON_COPIES - 80
CONE_RUN_MAX = 7
KERNEL = "DevModel_cfg3Lb0E"


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    """The device assembly of every kernel instance with its line table, compiled once for the module with the product build's flags."""
    out = tmp_path_factory.mktemp("isa") / "hsrsim.s"
    sys.path.insert(0, str(ROOT))
    from hsr_env_amd.build import CODEGEN_FLAGS
    subprocess.check_call([HIPCC, *CODEGEN_FLAGS, "-gline-tables-only", "-S", "--cuda-device-only", "-Wno-unused-result", "-Wno-unused-value",
                           "-o", str(out), str(ROOT / "hsr_env_amd" / "csrc" / "hsrsim.hip")], stderr=subprocess.DEVNULL)
    return out.read_text()


def cone_lines():
    """(first, last) line of the three cone functions in csrc/solve_g.h: from cone_eval2's signature to the line in front of what follows cone_dd."""
    src = (ROOT / "hsr_env_amd" / "csrc" / "solve_g.h").read_text().split("\n")
    first = next(k for k, t in enumerate(src, 1) if re.search(r"\bvoid cone_eval2\(", t))
    last = next(k for k, t in enumerate(src, 1) if k > first and t.startswith("enum { NLMAX"))
    assert any("void cone_dd(" in t for t in src[first:last])
    return first, last - 1


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not available")
def test_plain_copies_of_the_cfg3_newton_window(listing):
    name, ins = isa_slots.kernel_body(listing, KERNEL)
    lo, hi = isa_slots.newton_window(ins, 1500)
    n, copies, in_runs, nruns, cnd = isa_copies.counts(ins[lo:hi])
    print(name, "newton window:", n, "instructions,", copies, "plain copies,", in_runs, "in", nruns, "runs of five or more,", cnd, "v_cndmask; kernel:", isa_copies.counts(ins)[1], "copies")
    assert n > 2000, (name, lo, hi)          # the window was found
    assert copies <= NEWTON_COPIES_MAX, (copies, isa_copies.runs(ins[lo:hi]))


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not available")
def test_no_run_of_copies_in_the_cone_functions(listing):
    name, ins = isa_slots.kernel_body(listing, KERNEL)
    locs = isa_copies.kernel_locs(listing, KERNEL)
    assert locs is not None and len(locs) == len(ins), "the listing carries no line table"
    first, last = cone_lines()
    # an instruction the compiler made up (line 0) belongs to the last source line seen before it
    where, cur = [], ("?", 0)
    for (f, l), _ in locs:
        if l > 0: cur = (f, l)
        where.append(cur)
    assert sum(f == "solve_g.h" and first <= l <= last for f, l in where) > 300, "the cone functions were not found in the line table"
    lo, hi = isa_slots.newton_window(ins, 1500)
    bad = [(a, n, where[a]) for a, n in isa_copies.runs(ins, CONE_RUN_MAX + 1)
           if lo <= a < hi and any(f == "solve_g.h" and first <= l <= last for f, l in where[a:a + n])]
    assert not bad, bad
