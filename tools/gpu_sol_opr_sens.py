#!/usr/bin/env python3
"""How accurate radtran_sol_spectra_opr_vjp's kernels are, and what the call costs, on the GPU.

1. Accuracy: what tests/test_gpu_sol_opr_sens.py::test_hook_columns_against_exact runs (clima_test_sol_opr_sens on the
   stored columns of tests/golden/exact_sol_opr_sens_0.npz, 1 and 8 g-points; tests/sol_opr_sens_cases.py, no mpmath): per
   column and derivative array the kernel's and the reference restatement's largest error, and the worst error / allowed
   per parameter.
2. Cost, at config 2's shape and at 102 layers x 400 bins, medians of `--repeats` calls in one process:
     (a) sol_spectra_opr_vjp, one level (TOA, up), tau, w0, g and albedo -- the host form
     (b) sol_spectra_opr_vjp, 16 levels, up, down and amean
     (c) sol_spectra_opr_vjp_tensors, one level, sync=True: the device form of (a)
     (d) ir_spectra_opr_vjp_tensors, one level: the IR counterpart
     (e) radiate_solar_batch, one case
     (f) radiate(compute_opacity=True): the single call, which this work must not move
3. `--single-call`: (f) alone at both shapes, for whichever build CLIMA_HIP_LIB names -- run once per build, alternating,
   in one session, to set this build's single call beside the parent commit's.

  python tools/gpu_sol_opr_sens.py [--out FILE] [--repeats 9] [--small] [--single-call]
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
ap.add_argument("--single-call", action="store_true")
args = ap.parse_args()

import sol_opr_sens_cases as K  # noqa: E402
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
    say("clima_test_sol_opr_sens against exact derivatives (tests/golden/exact_sol_opr_sens_0.npz)")
    say("kernel, reference: largest |value - exact| of the array, as a fraction of its largest exact magnitude")
    say("criterion of the tests: kernel <= max(%.0e, %.0f x reference)" % (K.FLOOR, K.MARGIN))
    for ng in (1, 8):
        recs, ran, nonzero = K.run(L, E, ng)
        say("")
        say("ng = %d, %d columns" % (ng, ran))
        say("  %-6s %-26s %-8s %10s %10s %s" % ("column", "shape", "array", "kernel", "reference", ""))
        for r in recs:
            s = r.scale if r.scale > 0 else 1.0
            say("  %-6s %-26s %-8s %10.2e %10.2e %s" % (r.name, r.group, r.quantity, r.err / s, r.e_ref / s, "" if r.ok else "FAILS"))
        say("  worst kernel error / allowed error: " + ", ".join("d/d%s %.2g" % kv for kv in K.worst_ratios(recs).items()))
        say("  identically-zero exact arrays that did not come back as zeros: %s" % (", ".join(nonzero) or "none"))


def row(name, seconds):
    ms = [1e3 * x for x in seconds]
    med = statistics.median(ms)
    say("  %-84s median %9.3f ms  (min %9.3f  max %9.3f)" % (name, med, min(ms), max(ms)))
    return med


def measure(title, tables, col, repeats):
    import torch
    nz = len(col["T"])
    r = Radtran(tables, nz, 4, 0.15)
    r.radiate(*col.args())
    Ts, T = col["T_surface"], np.asarray(col["T"], dtype=float)
    nw_sol, nw_ir = len(r.sol.freq) - 1, len(r.ir.freq) - 1
    lv16 = np.linspace(0, nz, 16).astype(int)
    one = dict(fup=np.ones((nw_sol, 1)))
    many = {k: np.ones((nw_sol, 16)) for k in ("fup", "fdn", "amean")}
    dev = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")   # noqa: E731
    d_one, d_Ts, d_T, d_ir = dict(fup=dev(one["fup"].T)), dev([Ts]), dev(T), dict(fup=dev(np.ones((1, nw_ir))))
    zu, zw = np.array(r.zenith_u)[None, :], np.array(r.zenith_weights)[None, :]
    variants = [("(a) sol_spectra_opr_vjp, 1 level (TOA, up)", lambda: r.sol_spectra_opr_vjp(one, (-1,))),
                ("(b) sol_spectra_opr_vjp, 16 levels, up, down and amean", lambda: r.sol_spectra_opr_vjp(many, lv16)),
                ("(c) sol_spectra_opr_vjp_tensors, 1 level, device arrays", lambda: r.sol_spectra_opr_vjp_tensors(d_one, (-1,), sync=True)),
                ("(d) ir_spectra_opr_vjp_tensors, 1 level, device arrays", lambda: r.ir_spectra_opr_vjp_tensors(d_Ts, d_T, d_ir, (-1,), sync=True)),
                ("(e) radiate_solar_batch, 1 case", lambda: r.radiate_solar_batch(zu, zw)),
                ("(f) radiate, compute_opacity=True (the single call)", lambda: (r.radiate(*col.args()), r.synchronize()))]
    for _, fn in variants:
        fn()
    say("%s: %d layers, %d solar bins x %d g-points, %d zenith angles; library %s" % (
        title, nz, nw_sol, len(tables.ktables[0]["weights"]), zu.shape[1], os.path.relpath(lib.LIB_PATH)))
    times = {name: [] for name, _ in variants}
    for _ in range(repeats):
        for name, fn in variants:
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    med = [row(name, times[name]) for name, _ in variants]
    say("  (b) / (a) = %.2f; (c) / (d) = %.2f; (c) / (e) = %.2f; (a) - (c) = %.3f ms" % (med[1] / med[0], med[2] / med[3], med[2] / med[4], med[0] - med[2]))


def single_call(title, tables, col, repeats):
    nz = len(col["T"])
    r = Radtran(tables, nz, 4, 0.15)
    fn = lambda: (r.radiate(*col.args()), r.synchronize())   # noqa: E731
    for _ in range(3):
        fn()
    t = []
    for _ in range(6 * repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    row("(f) radiate, %s; library %s" % (title, os.path.relpath(lib.LIB_PATH)), t)


if args.single_call:
    # (a build of an earlier commit does not export every entry point the ctypes table names: this mode calls radiate alone)
    import ctypes
    probe = ctypes.CDLL(lib.LIB_PATH)
    for name in [n for n in lib.SIGNATURES if not hasattr(probe, n)]:
        del lib.SIGNATURES[name]
else:
    accuracy()
    say("")
if args.small:
    shapes = [("small A", S.modern_earth_tables(nw=60), S.modern_earth_column(40)),
              ("small B", S.modern_earth_tables(nw=40), S.Column(copy_atm_to_radiative_grid(S.modern_earth_column(15))))]
else:
    shapes = [("config 2's column", S.modern_earth_tables(), S.modern_earth_column(200)),
              ("102 layers x 400 bins", S.modern_earth_tables(nw=400), S.Column(copy_atm_to_radiative_grid(S.modern_earth_column(50))))]
for title, tables, col in shapes:
    (single_call if args.single_call else measure)(title, tables, col, args.repeats)
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
