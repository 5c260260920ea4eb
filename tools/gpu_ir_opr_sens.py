#!/usr/bin/env python3
"""How accurate radtran_ir_spectra_opr_vjp's kernels are, and what the call costs, on the GPU.

1. Accuracy: what tests/test_gpu_ir_opr_sens.py::test_hook_columns_against_exact runs (clima_test_ir_opr_sens on the
   stored columns of tests/golden/exact_ir_opr_sens_0.npz, 1 and 8 g-points; tests/ir_opr_sens_cases.py, no mpmath): per
   column and derivative array the kernel's error and the reference algorithm's, as fractions of the array's scale, and per
   parameter the worst kernel error over the allowed one.
2. Time, at config 2's shape (200 layers) and at 102 layers x 400 bins, in ONE process, alternating the variants,
   `--repeats` timed repeats each after one warm-up of every variant:
     (a) ir_spectra_opr_vjp, one level (top of the atmosphere, up), tau, w0 and g
     (b) ir_spectra_opr_vjp, 16 levels, up and down
     (c) ir_jacobian_spectral, one row (top, up): radtran_ir_jacobian_spectral_rows, the same per-(bin, g-point) structure
     (d) ir_spectra_opr_vjp_tensors, one level, sync=True: the device form of (a) -- the same kernels, nothing copied
   Times are host clocks around synchronous calls.  (a) and (b) return tau's and w0's whole arrays (nz x ngauss x nw
   doubles each) through the pinned block, (c) one row of nw_ir x (nz + 1): (a) - (d) is what the copies cost.

  python tools/gpu_ir_opr_sens.py [--out FILE] [--repeats 9] [--small]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--small", action="store_true")
args = ap.parse_args()

import ir_opr_sens_cases as K  # noqa: E402
from clima_amd import lib  # noqa: E402
from clima_amd import synthetic as S  # noqa: E402
from clima_amd.atmosphere import copy_atm_to_radiative_grid  # noqa: E402
from clima_amd.radtran import Radtran  # noqa: E402

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def accuracy():
    L, E = lib.load(), K.load()
    say("clima_test_ir_opr_sens against exact derivatives (tests/golden/exact_ir_opr_sens_0.npz)")
    say("kernel, reference: largest |value - exact| of the array, as a fraction of its largest exact magnitude")
    say("criterion of the tests: kernel <= max(%.0e, %.0f x reference)" % (K.FLOOR, K.MARGIN))
    for ng in (1, 8):
        recs, ran = K.run(L, E, ng)
        say("")
        say("ng = %d, %d columns" % (ng, ran))
        say("  %-6s %-16s %-7s %10s %10s %s" % ("column", "shape", "array", "kernel", "reference", ""))
        for r in recs:
            s = r.scale if r.scale > 0 else 1.0
            say("  %-6s %-16s %-7s %10.2e %10.2e %s" % (r.name, r.group, r.quantity, r.err / s, r.e_ref / s, "" if r.ok else "FAILS"))
        say("  worst kernel error / allowed error: " + ", ".join("d/d%s %.2g" % kv for kv in K.worst_ratios(recs).items()))


def row(name, seconds):
    ms = [1e3 * x for x in seconds]
    med = statistics.median(ms)
    say("  %-58s median %9.3f ms  (min %9.3f  max %9.3f)" % (name, med, min(ms), max(ms)))
    return med


def measure(title, tables, col, repeats):
    nz = len(col["T"])
    r = Radtran(tables, nz, 4, 0.15)
    r.radiate(*col.args())
    Ts, T = col["T_surface"], np.asarray(col["T"], dtype=float)
    nw_ir = len(r.ir.freq) - 1
    lv16 = np.linspace(0, nz, 16).astype(int)
    one = dict(fup=np.ones((nw_ir, 1)))
    many = dict(fup=np.ones((nw_ir, 16)), fdn=np.ones((nw_ir, 16)))
    import torch
    dev = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")   # noqa: E731
    d_Ts, d_T, d_one = dev([Ts]), dev(T), dict(fup=dev(one["fup"].T))
    variants = [("(a) ir_spectra_opr_vjp, 1 level (TOA, up)", lambda: r.ir_spectra_opr_vjp(Ts, T, one, (-1,))),
                ("(b) ir_spectra_opr_vjp, 16 levels, up and down", lambda: r.ir_spectra_opr_vjp(Ts, T, many, lv16)),
                ("(c) ir_jacobian_spectral, 1 row (TOA, up)", lambda: r.ir_jacobian_spectral(Ts, T)),
                ("(d) ir_spectra_opr_vjp_tensors, 1 level, device arrays", lambda: r.ir_spectra_opr_vjp_tensors(d_Ts, d_T, d_one, (-1,), sync=True))]
    for _, fn in variants:
        fn()
    say("%s: %d layers, %d IR bins x %d g-points; library %s" % (title, nz, nw_ir, len(tables.ktables[0]["weights"]), os.path.relpath(lib.LIB_PATH)))
    times = {name: [] for name, _ in variants}
    for _ in range(repeats):
        for name, fn in variants:
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    med = [row(name, times[name]) for name, _ in variants]
    mb = 8.0e-6 * (2 * nz * len(tables.ktables[0]["weights"]) * r.nw + nz * r.nw)
    say("  (a) / (c) = %.2f; (b) / (a) = %.2f; (d) / (c) = %.2f; (a) - (d) = %.3f ms for %.1f MB of results" % (
        med[0] / med[2], med[1] / med[0], med[3] / med[2], med[0] - med[3], mb))


accuracy()
say("")
if args.small:
    shapes = [("small A", S.modern_earth_tables(nw=60), S.modern_earth_column(40)),
              ("small B", S.modern_earth_tables(nw=40), S.Column(copy_atm_to_radiative_grid(S.modern_earth_column(15))))]
else:
    shapes = [("config 2's column", S.modern_earth_tables(), S.modern_earth_column(200)),
              ("102 layers x 400 bins", S.modern_earth_tables(nw=400), S.Column(copy_atm_to_radiative_grid(S.modern_earth_column(50))))]
for title, tables, col in shapes:
    measure(title, tables, col, args.repeats)
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
