#!/usr/bin/env python3
"""tools/compare_kernel_asm.py A.s B.s — is the device code of two builds of a .hip file the same, function by function?

Both files are device-only assembly of the same source at two revisions, compiled with the flags of lp_mp_amd/build.py:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-strict-aliasing --cuda-device-only -S kernels.hip -o A.s

Functions are keyed by symbol, because the order in which templates are instantiated (and with it the order of the file and
the numbers in the compiler's local labels) changes with harmless edits of the host code.  Per symbol the instruction text
and, for kernels, the .amdhsa_* resource lines (VGPRs, SGPRs, LDS, scratch) are compared.  The __hip_cuid_<hash> symbol is a
hash of the source text and is ignored.  Prints the symbols only in one file, the symbols whose text differs, and
"identical" otherwise; the exit status is 0 only for "identical"."""
import re
import sys

LOCAL = re.compile(r"\.L(BB|func_begin|func_end|tmp|JTI|CPI)\d+(_\d+)?")


def normalise(line):
    # local labels carry the function's index in the file: .LBB12_3 -> .LBB_3
    return LOCAL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), line.split(";")[0].rstrip())


def parse(path):
    text, res, name, desc = {}, {}, None, None
    with open(path) as fh:
        for raw in fh:
            line = raw.strip()
            if "__hip_cuid_" in line:
                continue
            m = re.match(r"\.amdhsa_kernel\s+(\S+)", line)   # (the descriptor sits between a kernel's last instruction and its .size)
            if m:
                desc = m.group(1)
                res[desc] = []
            elif line.startswith(".end_amdhsa_kernel"):
                desc = None
            elif desc is not None:
                res[desc].append(normalise(line))
            elif re.match(r"\.type\s+(\S+),@function", line):
                name = re.match(r"\.type\s+(\S+),@function", line).group(1)
                text[name] = []
            elif line.startswith(".size"):
                name = None
            elif name is not None and not line.startswith(".Lfunc_end") and normalise(line):
                text[name].append(normalise(line))
    return text, res


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    (ta, ra), (tb, rb) = parse(sys.argv[1]), parse(sys.argv[2])
    bad = 0
    for what, a, b in (("function", ta, tb), ("kernel descriptor", ra, rb)):
        for s in sorted(set(a) - set(b)):
            print("only in %s: %s %s" % (sys.argv[1], what, s)); bad += 1
        for s in sorted(set(b) - set(a)):
            print("only in %s: %s %s" % (sys.argv[2], what, s)); bad += 1
        for s in sorted(set(a) & set(b)):
            if a[s] != b[s]:
                first = next((i for i, (x, y) in enumerate(zip(a[s], b[s])) if x != y), min(len(a[s]), len(b[s])))
                print("differs: %s %s (%d / %d lines, first difference at line %d)" % (what, s, len(a[s]), len(b[s]), first)); bad += 1
    if bad:
        sys.exit(1)
    print("identical: %d functions, %d kernels (%d instruction lines)" % (len(ta), len(ra), sum(len(v) for v in ta.values())))


if __name__ == "__main__":
    main()
