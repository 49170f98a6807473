#!/usr/bin/env python3
"""Are two sets of gfx950 assembly files the same device code, function by function?  For a change that only MOVES kernels between sources.

  hipcc $(HIPFLAGS) --cuda-device-only -S -Iraytracers_amd/csrc raytracers_amd/csrc/render_kernels.hip -o before.s      (at the old commit)
  ... the same for every kernel source of the new commit, then
  tools/kernel_asm_diff.py --before before.s --after render.s query.s

Compared per symbol of type @function: the instruction text between its label and its .Lfunc_end (comment lines dropped, local labels such
as .LBB<n>_<m> renumbered without the function's index n, which depends on its place in the file), and for a kernel the lines of its
.amdhsa_kernel block (registers, LDS, scratch).  The union of each side must be the same symbols.  Exit status 1 on any difference."""
import argparse
import re
import sys

LOCAL = re.compile(r"\.L([A-Za-z_]+?)\d+(_\d+)?\b")


def functions(paths):
    body, desc = {}, {}
    for path in paths:
        lines = open(path).read().split("\n")
        names = [m.group(1) for m in (re.match(r"\s*\.type\s+(\S+),@function", l) for l in lines) if m]
        at = {m.group(1): i for i, m in enumerate(re.match(r"([^\s.;][^\s:]*):", l) for l in lines) if m}
        for name in names:
            out = []
            for l in lines[at[name] + 1:]:
                if l.startswith(".Lfunc_end"):
                    break
                s = l.split(";")[0].strip()   # (comments: whole lines, and the loop notes behind labels)
                if s:
                    out.append(LOCAL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), s))
            assert name not in body or body[name] == out, f"{name}: defined twice, differently"
            body[name] = out
        for i, l in enumerate(lines):
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
            if m:
                end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
                desc[m.group(1)] = [x.strip() for x in lines[i + 1:end]]
    return body, desc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--before", nargs="+", required=True)
    ap.add_argument("--after", nargs="+", required=True)
    a = ap.parse_args()
    (b0, d0), (b1, d1) = functions(a.before), functions(a.after)
    bad = []
    for name in sorted(set(b0) ^ set(b1)):
        bad.append(f"only {'before' if name in b0 else 'after'}: {name}")
    for name in sorted(set(b0) & set(b1)):
        if b0[name] != b1[name]:
            bad.append(f"instructions differ: {name} ({len(b0[name])} -> {len(b1[name])} lines)")
        elif d0.get(name) != d1.get(name):
            bad.append(f"kernel descriptor differs: {name}")
    print("\n".join(bad), end="\n" if bad else "")
    same = [n for n in set(b0) & set(b1) if b0[n] == b1[n] and d0.get(n) == d1.get(n)]
    print(f"kernels: {len(d0)} before, {len(d1)} after; identical: {sum(n in d0 for n in same)} kernels, "
          f"{sum(n not in d0 for n in same)} device functions; different: {len(bad)}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
