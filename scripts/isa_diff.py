#!/usr/bin/env python3
"""Development aid: do two builds hold the same device code, kernel by kernel, whatever file a kernel sits in?
  hipcc <the Makefile's flags for the file> --offload-device-only -S file.hip -o file.s      (every file of both sides)
  scripts/isa_diff.py --old a.s b.s --new c.s d.s e.s
Per kernel symbol: the text from its label to .Lfunc_end (instructions and the .amdhsa_kernel descriptor), with the function index
of local labels (.LBB<n>_, .Lfunc_end<n>, ...) dropped, .Ltmp<n> numbered from the kernel's first one, and `;` comments stripped.
Prints the kernels that differ, are missing on a side or occur more than once on a side; exit status 1 if there is any."""
import argparse
import re
import sys


def kernels(paths):
    out = {}
    for path in paths:
        lines = open(path).read().split("\n")
        for sym in (m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m):
            i = lines.index(next(l for l in lines if l.startswith(sym + ":")))
            j = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
            text, tmps = [], {}
            for l in lines[i:j]:
                l = re.sub(r"\.L([A-Za-z_]+?)\d+_", r".L\1_", l.split(";")[0].rstrip())
                l = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", l)
                l = re.sub(r"\.Ltmp\d+", lambda m: ".Ltmp%d" % tmps.setdefault(m.group(0), len(tmps)), l)
                if l.strip():
                    text.append(l)
            out.setdefault(sym, []).append((path, text))
    return out


ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--old", nargs="+", required=True)
ap.add_argument("--new", nargs="+", required=True)
a = ap.parse_args()
old, new = kernels(a.old), kernels(a.new)
bad = 0
for sym in sorted(set(old) | set(new)):
    o, n = old.get(sym, []), new.get(sym, [])
    if len(o) != 1 or len(n) != 1:
        what = "old: %s, new: %s" % ([p for p, _ in o] or "missing", [p for p, _ in n] or "missing")
    elif o[0][1] != n[0][1]:
        what = "DIFFERS (%d / %d lines)" % (len(o[0][1]), len(n[0][1]))
    else:
        print("same     %-6d lines  %-28s %s" % (len(n[0][1]), n[0][0].split("/")[-1], sym))
        continue
    bad += 1
    print("PROBLEM  %s: %s" % (sym, what))
print("%d kernels old, %d new, %d problems" % (len(old), len(new), bad))
sys.exit(1 if bad else 0)
