"""Issue slots spent on plain register copies, for one kernel of an `-S` listing: python tools/isa_copies.py LISTING.s SYMBOL-SUBSTRING [--all | --lines FILE:A-B[,FILE:A-B..]]
LISTING.s and the kernel as for tools/isa_slots.py (whose kernel_body / newton_window this uses); compiled with -gline-tables-only added,
the listing carries `.loc` lines, which change no instruction, and every run is printed with the source line it belongs to.

A plain copy is a `v_mov_b32` the compiler wrote that is neither a DPP nor an SDWA form: a register-to-register move or the load of a
constant.  It does no arithmetic, and a wave that is alone on its SIMD pays a full issue slot for it.  Runs of them are what a merge of
values across a branch looks like (a struct zero-initialised and then filled per arm, a loop-carried set of registers, `x = y` followed
by `x += ...`), so the runs of RUN_MIN or more are listed with their position.

Printed: instructions, plain copies and v_cndmask of the whole kernel and of the Newton window; copies in runs of RUN_MIN or more; the runs
(index of the first copy, length, `in window`), each with the innermost source line of its first copy and - as tools/isa_map.py attributes
instructions - the last line of persist.h / solve_body.inc seen before it; with --all also the runs outside the window's neighbourhood.

--lines collide.h:242-326,collide.h:711-886 (listing with `.loc` lines): instead of the above, one row per INNERMOST source line inside the given
ranges - instructions, plain copies, v_cndmask, SALU, SALU that touches the exec mask, branches, wait states - a total per file, and the sum
copies + wait states + exec-mask SALU (the slots without arithmetic that tests/test_isa_mpr.py bounds for the MPR functions)."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_slots  # noqa: E402

RUN_MIN = 5
TOP = ("persist.h", "solve_body.inc")
PLAIN = ("v_mov_b32", "v_mov_b32_e32", "v_mov_b32_e64")


def is_copy(i) -> bool:
    return i.op in PLAIN and not i.hand


def runs(ins, run_min=RUN_MIN):
    """[(index of the first copy, length)] of the runs of at least run_min consecutive plain copies."""
    out, k = [], 0
    while k < len(ins):
        if not is_copy(ins[k]):
            k += 1; continue
        a = k
        while k < len(ins) and is_copy(ins[k]): k += 1
        if k - a >= run_min: out.append((a, k - a))
    return out


def counts(ins):
    """(instructions, plain copies, copies in runs of RUN_MIN or more, number of such runs, v_cndmask)"""
    r = runs(ins)
    return len(ins), sum(is_copy(i) for i in ins), sum(n for _, n in r), len(r), sum(i.op.startswith("v_cndmask") for i in ins)


def kernel_locs(listing: str, symbol: str):
    """Per instruction of isa_slots.kernel_body(listing, symbol): ((file, line) innermost, (file, line) of the last TOP file seen), or
    None when the listing has no .loc lines.  File names are base names."""
    files = {}
    for m in re.finditer(r"^\s*\.file\s+(\d+)\s+((?:\"[^\"]*\"\s*)+)", listing, flags=re.M):
        files[int(m.group(1))] = os.path.basename(re.findall(r"\"([^\"]*)\"", m.group(2))[-1])
    m = re.search(r"^(\w*" + re.escape(symbol) + r"\w*):[^\n]*\n(.*?)s_endpgm", listing, flags=re.S | re.M)
    if not m or ".loc" not in m.group(2):
        return None
    out, cur, top = [], ("?", 0), ("?", 0)
    for t in m.group(2).split("\n"):
        t = t.strip()
        l = re.match(r"\.loc\s+(\d+)\s+(\d+)", t)
        if l:
            cur = (files.get(int(l.group(1)), "?"), int(l.group(2)))
            if cur[0] in TOP and cur[1] > 0: top = cur
            continue
        if not t or t.startswith((".", ";", "//")) or t.endswith(":"):
            continue
        out.append((cur, top))
    return out


def innermost(locs):
    """(file, line) of the innermost source line per instruction; an instruction the compiler made up (line 0) belongs to the last line seen before it."""
    out, cur = [], ("?", 0)
    for (f, l), _ in locs:
        if l > 0: cur = (f, l)
        out.append(cur)
    return out


def parse_lines(spec: str):
    """'collide.h:711-886,persist.h:534-619' -> [(file, first, last)]"""
    out = []
    for part in spec.split(","):
        f, _, r = part.partition(":")
        a, _, b = r.partition("-")
        out.append((f, int(a), int(b or a)))
    return out


def is_exec_salu(i) -> bool:
    """scalar instruction that reads or writes the exec mask (what a divergent branch or a select under a lane condition is made of)"""
    return i.op.startswith("s_") and not i.op.startswith(("s_cbranch", "s_branch", "s_waitcnt", "s_nop")) and ("saveexec" in i.op or "exec" in i.text.split(None, 1)[-1])


ACCOUNT = ("instr", "copies", "cndmask", "salu", "exec", "branches", "nop_ws")


def account(i):
    """this instruction's contribution to the columns of ACCOUNT (nop_ws: wait states, an `s_nop N` is N + 1)"""
    salu = i.op.startswith("s_") and not i.op.startswith(("s_cbranch", "s_branch", "s_waitcnt", "s_nop"))
    return (1, int(is_copy(i)), int(i.op.startswith("v_cndmask")), int(salu), int(is_exec_salu(i)), int(i.op.startswith(("s_cbranch", "s_branch"))),
            isa_slots.slots(i) if i.op == "s_nop" else 0)


def line_account(ins, locs, ranges):
    """{(file, line): [columns of ACCOUNT]} over the instructions whose innermost source line lies in one of `ranges` [(file, first, last)]."""
    rows = {}
    for i, (f, l) in zip(ins, innermost(locs)):
        if not any(f == rf and a <= l <= b for rf, a, b in ranges): continue
        row = rows.setdefault((f, l), [0] * len(ACCOUNT))
        for k, v in enumerate(account(i)): row[k] += v
    return rows


def no_work_slots(rows) -> int:
    """plain copies + wait states + exec-mask SALU of a line_account: issue slots that do no arithmetic (tests/test_isa_mpr.py bounds them)"""
    c, e, w = ACCOUNT.index("copies"), ACCOUNT.index("exec"), ACCOUNT.index("nop_ws")
    return sum(r[c] + r[e] + r[w] for r in rows.values())


def print_line_account(ins, locs, ranges):
    rows = line_account(ins, locs, ranges)
    print(f"{'innermost line':22s} " + " ".join(f"{c:>8s}" for c in ACCOUNT))
    tot = {}
    for (f, l), r in sorted(rows.items()):
        print(f"{f + ':' + str(l):22s} " + " ".join(f"{v:8d}" for v in r))
        t = tot.setdefault(f, [0] * len(ACCOUNT))
        for k, v in enumerate(r): t[k] += v
    for f, t in sorted(tot.items()):
        print(f"{f + ' (ranges)':22s} " + " ".join(f"{v:8d}" for v in t))
    print(f"copies + wait states + exec-mask SALU: {no_work_slots(rows)}")


def main(argv):
    if len(argv) < 3:
        raise SystemExit(__doc__)
    listing = open(argv[1]).read()
    name, ins = isa_slots.kernel_body(listing, argv[2])
    locs = kernel_locs(listing, argv[2])
    assert locs is None or len(locs) == len(ins)
    lines = [a for k, a in enumerate(argv) if k and (argv[k - 1] == "--lines" or a.startswith("--lines="))]
    if lines:
        assert locs is not None, "--lines needs a listing compiled with -gline-tables-only"
        print(name)
        print_line_account(ins, locs, parse_lines(lines[0].split("=", 1)[-1]))
        return
    tail = 3500 if "cfg4" in name else 1500
    lo, hi = isa_slots.newton_window(ins, tail)
    print(name)
    print(f"{'':14s} {'instr':>7s} {'copies':>7s} {'in runs':>8s} {'runs':>5s} {'cndmask':>8s}")
    for label, part in (("kernel", ins), ("newton window", ins[lo:hi])):
        n, cp, inr, nr, cnd = counts(part)
        print(f"{label:14s} {n:7d} {cp:7d} {inr:8d} {nr:5d} {cnd:8d}" + (f"      (instructions {lo} .. {hi}: first v_mfma to {tail} past the last)" if part is not ins else ""))
    print(f"\nruns of {RUN_MIN} or more plain copies (index of the first, length):")
    for a, n in runs(ins):
        inside = lo <= a < hi
        if not inside and "--all" not in argv: continue
        where = ""
        if locs:
            (f, l), (tf, tl) = locs[a]
            where = f"  {f}:{l}" + (f"  <- {tf}:{tl}" if (tf, tl) != (f, l) else "")
        print(f"  {a:6d} {n:3d} {'in window' if inside else '':9s}{where}")


if __name__ == "__main__":
    main(sys.argv)
