#!/usr/bin/env python3
"""kernel_identity.py A B — is the device code of two builds the same, kernel by kernel?

A and B are directories of device-only assembly, one .s per device translation unit (`make -C ray_tracer_webgl_amd/csrc
asm-device ASM_DIR=...`, the shipping flags).  For every function symbol of every unit — the kernels, and any device function
the compiler kept out of line — the instruction text and, for a kernel, the .amdhsa_* resource directives are compared line
for line.  Only lines naming __hip_cuid_ (the compilation unit's id, a hash that differs between any two compilations) are
ignored.  One line per symbol; exit status 1 on any difference, on a symbol or a unit that only one side has."""
import os
import re
import sys

FUNC = re.compile(r"^\s*\.type\s+([A-Za-z_$.][\w$.]*),@function")
END = re.compile(r"^\.Lfunc_end\d+:")


def symbols(path):
    """{symbol: (kind, instruction lines, .amdhsa_ lines)} of one assembly file"""
    lines = [l.rstrip() for l in open(path) if "__hip_cuid_" not in l]
    out = {}
    i = 0
    while i < len(lines):
        m = FUNC.match(lines[i])
        if not m:
            i += 1
            continue
        name, text, hsa, in_hsa = m.group(1), [], [], False
        i += 1
        while i < len(lines) and not END.match(lines[i]):
            l = lines[i]
            if l.strip().startswith(".amdhsa_kernel"):
                in_hsa = True
            if in_hsa:
                hsa.append(l)
            else:
                text.append(l)
            if l.strip() == ".end_amdhsa_kernel":
                in_hsa = False
            i += 1
        out[name] = ("kernel" if hsa else "function", text, hsa)
    return out


def main(a, b):
    units_a, units_b = (sorted(f for f in os.listdir(d) if f.endswith(".s")) for d in (a, b))
    bad = 0
    for unit in sorted(set(units_a) | set(units_b)):
        if unit not in units_a or unit not in units_b:
            print("%-24s only in %s" % (unit, a if unit in units_a else b))
            bad += 1
            continue
        sa, sb = symbols(os.path.join(a, unit)), symbols(os.path.join(b, unit))
        for name in sorted(set(sa) | set(sb)):
            if name not in sa or name not in sb:
                verdict = "ONLY IN " + (a if name in sa else b)
            else:
                (kind, ta, ha), (_, tb, hb) = sa[name], sb[name]
                what = [w for w, x, y in (("instructions", ta, tb), ("resources", ha, hb)) if x != y]
                verdict = "DIFFERS (%s)" % ", ".join(what) if what else "identical  %s, %d lines" % (kind, len(ta) + len(ha))
            bad += not verdict.startswith("identical")
            print("%-24s %-40s %s" % (unit, name, verdict))
    print("%s: %d difference(s)" % ("IDENTICAL" if not bad else "NOT IDENTICAL", bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
