#!/usr/bin/env python3
"""Developer diagnostic: scratch (register-spill) instructions per kernel of kernels.hip, from the gfx950
assembly.  A wave of these kernels stalls for an L2 round trip on every scratch reload, so builds that differ
only in where the register allocator spilled differ by several us per call: the hot
kernels should show no scratch instruction at all between their first and last lines.  The assembly is the one
tests/test_build_quality.py reads (tests/build_inspect.py: the flags of clima_amd/build.py).

  python tools/scratch_report.py [-D...] [regex on the mangled name]     (cross-compiles: no GPU needed, ~1 min)
"""
import os, re, subprocess, sys
root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [root, os.path.join(root, "tests")]
import build_inspect  # noqa: E402
flags = tuple(a for a in sys.argv[1:] if a.startswith("-"))
pat = ([a for a in sys.argv[1:] if not a.startswith("-")] + ["k_"])[0]
rows = []
for name, (n, hits) in build_inspect.kernel_scratch(flags).items():
    if re.search(pat, name):
        ld, st = (sum(what in line for _, line in hits) for what in ("scratch_load", "scratch_store"))
        rows.append((name, n, ld, st, [at for at, _ in hits]))
if not rows:
    sys.exit("no kernel matches %r" % pat)
dem = subprocess.run(["c++filt"] + [r[0] for r in rows], capture_output=True, text=True).stdout.split("\n")
for (name, n, ld, st, where), dn in zip(rows, dem):
    short = dn.split("(")[0].replace("void clima::", "")
    print("%-46s %6d lines  %3d scratch loads %3d stores  at %s" % (short, n, ld, st, " ".join(map(str, where[:24])) + (" ..." if len(where) > 24 else "")))
