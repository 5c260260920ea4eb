#!/usr/bin/env python3
"""What radtran_ir_jacobian_spectral_rows costs against the calls that form the same row, on the GPU.

At config 2's shape (200 layers) and at the 102- and 402-layer doubled grids (400 bins), in ONE process, alternating the
variants, `--repeats` timed repeats each after one warm-up of every variant:
  (a) ir_jacobian_spectral, one row (top of the atmosphere, up)
  (b) ir_jacobian_spectral, two rows (top and surface), up and down
  (c) ir_jacobian_reduced with the single row nz+1 and every x its own group: the cheapest existing call that forms the
      same row, summed over the bins
  (d) at 102 layers only, the route the new call replaces: 2 (nz+1) IR-only calls at x(j) +- h, each followed by the two
      spectra getters
Times are host clocks around synchronous calls.

  python tools/gpu_ir_jacobian_spectral.py [--out FILE] [--repeats 9] [--small]
  python tools/gpu_ir_jacobian_spectral.py --jacobian [--out FILE] [--repeats 25]

--small: tiny shapes, to rehearse the script.
--jacobian: time radtran_ir_jacobian at 200 layers alone (5 warm-up calls), for a library A/B under CLIMA_HIP_LIB: it uses
nothing a build without the new call lacks."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--repeats", type=int, default=None)
ap.add_argument("--small", action="store_true")
ap.add_argument("--jacobian", action="store_true")
args = ap.parse_args()

from clima_amd import lib  # noqa: E402
from clima_amd import synthetic as S  # noqa: E402
from clima_amd.atmosphere import copy_atm_to_radiative_grid  # noqa: E402
from clima_amd.radtran import Radtran  # noqa: E402

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def row(name, seconds, extra=""):
    ms = [1e3 * x for x in seconds]
    med = statistics.median(ms)
    say("  %-52s median %9.3f ms  (min %9.3f  max %9.3f)%s" % (name, med, min(ms), max(ms), extra))
    return med


def jacobian_alone(repeats):
    tables, col = S.modern_earth_tables(), S.modern_earth_column(200)
    r = Radtran(tables, 200, 4, 0.15)
    r.radiate(*col.args())
    for _ in range(5):
        r.ir_jacobian(col["T_surface"], col["T"])
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r.ir_jacobian(col["T_surface"], col["T"])
        t.append(time.perf_counter() - t0)
    say("radtran_ir_jacobian, config 2's column (200 layers, %d IR bins), %d calls; library %s"
        % (len(r.ir.freq) - 1, repeats, os.path.relpath(lib.LIB_PATH)))
    row("radtran_ir_jacobian", t)


def measure(title, tables, col, brute, repeats):
    nz = len(col["T"])
    r = Radtran(tables, nz, 4, 0.15)
    r.radiate(*col.args())
    Ts, T = col["T_surface"], np.asarray(col["T"], dtype=float)
    nw_ir = len(r.ir.freq) - 1
    groups = np.arange(1, nz + 2)
    x = np.concatenate([[Ts], T])

    def brute_force():
        out = np.empty((nw_ir, nz + 1))
        for j in range(nz + 1):
            h = 1.0e-4 * x[j]
            pair = []
            for s in (+1.0, -1.0):
                xp = x.copy()
                xp[j] += s * h
                r.radiate(xp[0], xp[1:], *col.args()[2:], compute_solar=False, compute_opacity=False)
                pair.append(np.array(r.wrk_ir.fup_a)[nz, :])
                np.array(r.wrk_ir.fdn_a)
            out[:, j] = (pair[0] - pair[1]) / (2 * h)
        return out

    variants = [("(a) ir_jacobian_spectral, 1 row (TOA, up)", lambda: r.ir_jacobian_spectral(Ts, T)),
                ("(b) ir_jacobian_spectral, 2 rows, up and down", lambda: r.ir_jacobian_spectral(Ts, T, levels=(-1, 0), parts=("up", "dn"))),
                ("(c) ir_jacobian_reduced, row nz+1, every x a group", lambda: r.ir_jacobian_reduced(Ts, T, groups, rows=[nz + 1], parts=True))]
    if brute:
        variants.append(("(d) 2 (nz+1) IR-only calls + getters", brute_force))
    got = {name: fn() for name, fn in variants}                   # the warm-up, and a look at the values
    names = [n for n, _ in variants]
    df = np.asarray(r.ir.freq, float)
    df = df[:-1] - df[1:]
    summed = (got[names[0]]["up"][:, 0, :] * df[:, None]).sum(axis=0)
    red = got[names[2]][0][0, :]
    say("%s: %d layers, %d IR bins x %d g-points; sum over the bins of (a) against (c): %.1e of the row's maximum; library %s"
        % (title, nz, nw_ir, len(tables.ktables[0]["weights"]), np.max(np.abs(summed - red)) / np.max(np.abs(red)),
           os.path.relpath(lib.LIB_PATH)))
    if brute:
        a, d = got[names[0]]["up"][:, 0, :], got[names[3]]
        say("  (d) against (a): %.1e of the slab's maximum" % (np.max(np.abs(a - d)) / np.max(np.abs(a))))
        r.radiate(*col.args(), compute_solar=False, compute_opacity=False)
    times = {name: [] for name in names}
    for _ in range(repeats):
        for name, fn in variants:
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    med = {name: row(name, times[name]) for name in names}
    say("  (a) / (c) = %.2f; (b) / (c) = %.2f%s" % (med[names[0]] / med[names[2]], med[names[1]] / med[names[2]],
                                                   "; (d) / (a) = %.0f" % (med[names[3]] / med[names[0]]) if brute else ""))


if args.jacobian:
    jacobian_alone(args.repeats or 25)
else:
    if args.small:
        shapes = [("small A", S.modern_earth_tables(nw=60), S.modern_earth_column(40), False),
                  ("small B", S.modern_earth_tables(nw=40), S.Column(copy_atm_to_radiative_grid(S.modern_earth_column(15))), True)]
    else:
        t400 = S.modern_earth_tables(nw=400)
        shapes = [("config 2's column", S.modern_earth_tables(), S.modern_earth_column(200), False),
                  ("102 layers x 400 bins", t400, S.Column(copy_atm_to_radiative_grid(S.modern_earth_column(50))), True),
                  ("402 layers x 400 bins", t400, S.Column(copy_atm_to_radiative_grid(S.modern_earth_column(200))), False)]
    for title, tables, col, brute in shapes:
        measure(title, tables, col, brute, args.repeats or 9)
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
