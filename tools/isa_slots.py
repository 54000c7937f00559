"""Issue slots that do no work, for one kernel of an `-S` listing: python tools/isa_slots.py LISTING.s SYMBOL-SUBSTRING [--dpp]
LISTING.s = `hipcc <CODEGEN_FLAGS of hsr_env_amd/build.py> -S --cuda-device-only` of csrc/hsrsim.hip; the kernel is the first symbol
that contains the substring (e.g. 'DevModel_cfg3Lb0E' for the plain cfg3 instance of k_env_step_mf).

Printed: instructions, s_nop count and wait states (an `s_nop N` is N + 1 wait states: a lone wave pays a full issue slot for each)
of the whole kernel and of the Newton window; the window's wait states by producer -> consumer class (the instruction in front of a
run of s_nop and the one behind it); wait states per 1000-instruction bucket; and for every DPP instruction the number of issue
slots between the last write of its DPP source register and the instruction itself.  gfx9 needs two between a VALU write and a DPP
read; the compiler pads what it emits itself, but it cannot see into an asm string, so the minimum over the HAND-WRITTEN DPP
instructions (those between ';;#ASMSTART' and ';;#ASMEND') is the safety figure (tests/test_isa_slots.py asserts it).

Instruction filter and Newton window are those of tests/test_isa_hazards.py: a line is an instruction unless it is empty, a
directive, a comment or a label; the window runs from the first v_mfma to TAIL instructions past the last one (1500; 3500 for cfg4)."""
import collections
import re
import sys

TRANS = ("v_rsq", "v_rcp", "v_sqrt", "v_exp", "v_log", "v_sin", "v_cos")
LOOKBACK = 64          # slots: a register written further back than this is no hazard of any kind


class Ins:
    __slots__ = ("text", "op", "hand")

    def __init__(self, text, hand):
        self.text, self.op, self.hand = text, text.split()[0], hand


def kernel_body(listing: str, symbol: str):
    """(name, instructions) of the first kernel whose symbol contains `symbol`."""
    m = re.search(r"^(\w*" + re.escape(symbol) + r"\w*):[^\n]*\n(.*?)s_endpgm", listing, flags=re.S | re.M)
    if not m:
        raise SystemExit(f"no kernel symbol contains {symbol!r}")
    ins, hand = [], False
    for t in m.group(2).split("\n"):
        t = t.strip()
        if t.startswith(";;#ASMSTART"): hand = True
        elif t.startswith(";;#ASMEND"): hand = False
        if not t or t.startswith((".", ";", "//")) or t.endswith(":"):
            continue
        ins.append(Ins(t, hand))
    return m.group(1), ins


def slots(i: Ins) -> int:
    return int(i.text.split()[1], 0) + 1 if i.op == "s_nop" else 1


def newton_window(ins, tail=1500):
    mf = [k for k, i in enumerate(ins) if i.op.startswith("v_mfma")]
    return (mf[0], min(len(ins), mf[-1] + tail)) if mf else (0, 0)


def counts(ins):
    nops = [i for i in ins if i.op == "s_nop"]
    return len(ins), len(nops), sum(slots(i) for i in nops)


def klass(i: Ins) -> str:
    if i.op.startswith("v_mfma"): return "MFMA"
    if "_dpp" in i.op or " row_" in i.text or " quad_perm" in i.text: return "DPP"
    if i.op.startswith(TRANS): return "TRANS"
    if i.op.startswith(("v_readlane", "v_writelane", "v_readfirstlane", "v_permlane")): return "LANE"
    if i.op.startswith("v_"): return "VALU"
    if i.op.startswith("s_"): return "SALU"
    return "MEM"


def by_context(ins):
    """{(producer class, consumer class): [runs of s_nop, wait states]}"""
    out = collections.defaultdict(lambda: [0, 0])
    k = 0
    while k < len(ins):
        if ins[k].op != "s_nop":
            k += 1; continue
        a = k
        while k < len(ins) and ins[k].op == "s_nop": k += 1
        key = (klass(ins[a - 1]) if a else "-", klass(ins[k]) if k < len(ins) else "-")
        out[key][0] += k - a; out[key][1] += sum(slots(i) for i in ins[a:k])
    return out


def regs(operand: str):
    """VGPR numbers named by one operand (v7, v[4:7]); empty for anything else."""
    m = re.match(r"v(\d+)$", operand)
    if m: return {int(m.group(1))}
    m = re.match(r"v\[(\d+):(\d+)\]$", operand)
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m else set()


def operands(i: Ins):
    parts = i.text.split(None, 1)
    return [o.strip().split()[0] for o in parts[1].split(",")] if len(parts) > 1 and parts[1].strip() else []


def written(i: Ins):
    """VGPRs the instruction writes."""
    ops = operands(i)
    if not ops or i.op.startswith(("s_", "v_cmp", "v_readlane", "v_readfirstlane", "global_store", "ds_write", "scratch_store", "buffer_store", "flat_store")):
        return set()
    w = regs(ops[0])
    if i.op.startswith("v_permlane") and "swap" in i.op and len(ops) > 1: w |= regs(ops[1])
    if i.op.startswith("v_swap") and len(ops) > 1: w |= regs(ops[1])
    return w


def dpp_distances(ins):
    """For every DPP instruction: (index, slots since the last write of its DPP source or None, class of the writer, hand-written?)."""
    out = []
    for k, i in enumerate(ins):
        if "_dpp" not in i.op: continue
        ops = operands(i)
        if len(ops) < 2: continue
        src = regs(ops[1])
        if not src: continue
        d, found = 0, None
        for p in range(k - 1, -1, -1):
            if written(ins[p]) & src:
                found = klass(ins[p]); break
            d += slots(ins[p])
            if d > LOOKBACK: break
        out.append((k, d if found else None, found, i.hand))
    return out


def min_hand_written_distance(ins):
    """Fewest issue slots between a VALU (or trans, or DPP) write of a register and a hand-written DPP read of it, with the offenders below two."""
    near = [(d, ins[k].text) for k, d, w, hand in dpp_distances(ins) if hand and d is not None and w in ("VALU", "DPP", "TRANS", "LANE")]
    return (min(d for d, _ in near) if near else None), [t for d, t in near if d < 2]


def main(argv):
    if len(argv) < 3:
        raise SystemExit(__doc__)
    name, ins = kernel_body(open(argv[1]).read(), argv[2])
    tail = 3500 if "cfg4" in name else 1500
    lo, hi = newton_window(ins, tail)
    win = ins[lo:hi]
    print(name)
    print(f"{'':14s} {'instr':>7s} {'s_nop':>6s} {'wait states':>12s}")
    print(f"{'kernel':14s} {counts(ins)[0]:7d} {counts(ins)[1]:6d} {counts(ins)[2]:12d}")
    print(f"{'newton window':14s} {counts(win)[0]:7d} {counts(win)[1]:6d} {counts(win)[2]:12d}      (instructions {lo} .. {hi}: first v_mfma to {tail} past the last)")
    print("\nwait states of the window by producer -> consumer:")
    for (a, b), (n, ws) in sorted(by_context(win).items(), key=lambda kv: -kv[1][1]):
        print(f"  {a:>5s} -> {b:5s} {n:5d} s_nop {ws:5d} wait states")
    print("\nwait states per 1000 instructions of the kernel:")
    for b in range(0, len(ins), 1000):
        print(f"  {b:6d} {counts(ins[b:b + 1000])[2]:5d}" + ("   <- newton window" if b < hi and b + 1000 > lo else ""))
    dist = dpp_distances(ins)
    hist = collections.Counter((hand, min(d, 8) if d is not None else -1) for _, d, _, hand in dist)
    print("\nDPP instructions by issue slots since the last write of their DPP source (8 = eight or more, - = none within reach):")
    for hand in (True, False):
        row = " ".join(f"{('-' if d < 0 else d)}:{hist[(hand, d)]}" for d in [-1] + list(range(9)) if hist[(hand, d)])
        print(f"  {'hand-written' if hand else 'compiler':13s} {row}")
    mn, bad = min_hand_written_distance(ins)
    print(f"safety figure (minimum over hand-written DPP reads of a VALU-written register): {mn}")
    for t in bad[:10]: print("  TOO CLOSE:", t)
    if "--dpp" in argv:
        for k, d, w, hand in dist: print(f"  {k:6d} {str(d):>4s} {str(w):5s} {'asm' if hand else '   '} {ins[k].text}")


if __name__ == "__main__":
    main(sys.argv)
