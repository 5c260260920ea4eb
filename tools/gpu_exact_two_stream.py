#!/usr/bin/env python3
"""How far the two-stream kernels are from the solution of the system, next to how far the reference algorithm is.

Runs what tests/test_gpu_exact_two_stream.py runs (the same fixtures, tests/golden/exact_two_stream_*.npz, the same
hooks, forms and measure: tests/exact_two_stream_cases.py; no mpmath) and prints, per hook, form and case group, the
kernels' worst error against exact, the reference algorithm's worst error against exact (the reference's stored output
where there is one and the oracle's two compilations), both as fractions of the quantity's scale, and their ratio.
Needs the GPU.  profiles/exact_two_stream.txt is its output.

    python tools/gpu_exact_two_stream.py > profiles/exact_two_stream.txt
"""
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import exact_two_stream_cases as XC  # noqa: E402


def table(title, recs):
    print()
    print(title)
    print("  %-34s %-46s %-15s %5s %10s %10s %8s %s" % ("form", "case group", "quantity", "n", "kernel", "reference", "ratio", "fails"))
    keys = []
    for r in recs:
        k = (r.form, r.group, r.quantity)
        if k not in keys:
            keys.append(k)
    for k in keys:
        mine = [r for r in recs if (r.form, r.group, r.quantity) == k]
        kern = max(r.err / r.scale for r in mine)
        ref = max(r.e_ref / r.scale for r in mine)
        ratio = "%8.2f" % (kern / ref) if ref > 0 else "     inf"
        print("  %-34s %-46s %-15s %5d %10.2e %10.2e %s %d" % (k + (len(mine), kern, ref, ratio, sum(not r.ok for r in mine))))


def main():
    from clima_amd import build, lib
    from oracle import oracle as O
    build.build()
    O.build()
    L = lib.load()
    G, E = XC.load_golden(), XC.load_exact()
    cols = XC.columns(G, E)
    cache = {}
    print("two-stream kernels against the exact solution of the system (tests/golden/exact_two_stream_*.npz)")
    print("kernel, reference: worst |value - exact| over the group, as a fraction of the quantity's scale; ratio: kernel / reference")
    print("criterion of the tests: kernel <= max(%.0e, %.0f x reference), record by record" % (XC.FLOOR, XC.MARGIN))
    recs = []
    for form, slots in ((0, 1), (0, 2), (0, 3), (1, 0), (2, 2), (2, 3), (3, None), (6, None), (4, 3), (4, 4), (4, 5), (5, 2), (5, 4)):
        recs += XC.run_two_stream(L, O, cols, form, slots, skip_512=form in (3, 6))[0]
    recs += XC.run_two_stream(L, O, cols, 0, 0, ng=1)[0]
    recs += XC.run_two_stream(L, O, [c for c in cols if XC.natural_slots(c) > 3], 2, None)[0]
    table("clima_test_two_stream (the direct two-stream)", recs)
    allr = recs
    recs = []
    for ng in (8, 1, 12):
        for force_nw in (0, 4):
            recs += XC.run_solar_batch_columns(L, O, cols, ng, force_nw)[0]
            recs += XC.run_solar_batch_multi(L, O, E, ng, force_nw, cache)[0]
    table("clima_test_solar_batch (k_twostream_sol_batch)", recs)
    allr += recs
    recs = []
    for ng in (1, 8):
        recs += XC.run_adjoint(L, O, E, ng, cache)[0]
    table("clima_test_ir_adjoint (ir_adjoint.inc)", recs)
    allr += recs
    recs = []
    for ng in (8, 3):
        recs += XC.run_response_golden(L, O, G, E, ng, cache)[0]
        recs += XC.run_response_deviations(L, O, E, ng, cache)[0]
    table("clima_test_ir_response (ir_green.inc)", recs)
    allr += recs
    print()
    print("columns singled out (every hook and form that ran them)")
    for title, pick in (("golden c21 IR", lambda r: r.name.startswith("c21") and r.quantity == "ir"),
                        ("golden c33 IR", lambda r: r.name.startswith("c33") and r.quantity == "ir"),
                        ("resonance columns, fluxes", lambda r: "res-" in r.name and r.quantity == "sol"),
                        ("resonance columns, amean", lambda r: "res-" in r.name and r.quantity == "amean"),
                        ("  of these off = 1e-8, fluxes", lambda r: "-1e-08" in r.name and r.quantity == "sol"),
                        ("  of these off = 1e-8, amean", lambda r: "-1e-08" in r.name and r.quantity == "amean"),
                        ("multi-angle case 0, fluxes", lambda r: r.name.startswith("m") and r.name.endswith("case 0") and r.quantity == "sol")):
        mine = [r for r in allr if pick(r)]
        kern, ref = [r.err / r.scale for r in mine], [r.e_ref / r.scale for r in mine]
        print("  %-28s %5d runs  kernel %.2e ... %.2e  reference %.2e ... %.2e  worst kernel / reference of one run %.2f" % (
            title, len(mine), min(kern), max(kern), min(ref), max(ref), max(a / b if b > 0 else (0.0 if a == 0 else float("inf")) for a, b in zip(kern, ref))))
    bad = XC.failures(allr)
    print()
    print("%d records, %d outside the criterion" % (len(allr), len(bad)))
    for r in bad[:40]:
        print("  ", r)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
