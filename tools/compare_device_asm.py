#!/usr/bin/env python3
"""Show that a host-side change left the device code alone: compare two device assemblies of hsrsim.hip function by function.

    hipcc <hsr_env_amd.build.CODEGEN_FLAGS> -S --cuda-device-only -o before.s hsr_env_amd/csrc/hsrsim.hip     (at the old commit)
    hipcc <hsr_env_amd.build.CODEGEN_FLAGS> -S --cuda-device-only -o after.s  hsr_env_amd/csrc/hsrsim.hip     (at the new one)
    python tools/compare_device_asm.py before.s after.s

Same set of function symbols and .amdhsa_kernel descriptors on both sides; per symbol an identical instruction stream and identical
.amdhsa_* directives (registers, scratch, LDS).  The order of the functions in the file and the numbers in local labels (.LBB12_3) may
differ: labels are renumbered per function by first appearance.  Exit status 1 if anything else differs.  Run it for the plain build
and for -DHSR_PHASE_TIMING."""
import re
import sys

LOCAL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def parse(path):
    funcs, kernels = {}, {}
    pending = cur = kern = None
    for raw in open(path):
        line = raw.split(";")[0].strip()                   # comments carry block numbers (; %bb.3:)
        if not line:
            continue
        m = re.match(r"\.type\s+(\S+),@function", line)
        if m:
            pending = m.group(1)
        elif pending and line == pending + ":":
            cur, pending, labels = funcs.setdefault(line[:-1], []), None, {}
        elif line.startswith(".amdhsa_kernel "):           # the descriptor sits between the kernel's code and its .Lfunc_end
            kern = kernels.setdefault(line.split()[1], [])
        elif line == ".end_amdhsa_kernel":
            kern = None
        elif kern is not None:
            kern.append(line)
        elif re.match(r"\.Lfunc_end\d+:", line):
            cur = None
        elif cur is not None:
            cur.append(LOCAL.sub(lambda t: labels.setdefault(t.group(0), f".L{len(labels)}"), line))
    return funcs, kernels


def main(a, b):
    (fa, ka), (fb, kb) = parse(a), parse(b)
    bad = []
    for what, x, y in (("function", fa, fb), ("kernel descriptor", ka, kb)):
        for name in sorted(set(x) | set(y)):
            if name not in x or name not in y:
                bad.append(f"{what} {name}: only in {a if name in x else b}")
            elif x[name] != y[name]:
                at = next((i for i, (p, q) in enumerate(zip(x[name], y[name])) if p != q), min(len(x[name]), len(y[name])))
                bad.append(f"{what} {name}: differs at line {at} of {len(x[name])} / {len(y[name])}")
    print("\n".join(bad) if bad else "", end="\n" if bad else "")
    print(f"{len(ka)} kernels, {len(fa)} functions, {sum(map(len, fa.values()))} instruction lines compared: {len(bad)} differing")
    return 1 if bad or not ka else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
